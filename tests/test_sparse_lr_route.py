"""The sparse-LR trainer's layout routing (pure host logic) and its construction-time
config checks."""
import pytest

from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
from parameter_server_amd.models.sparse_lr import _CSR_MAX_ROWS, route

B, W = 256, 39
NNZ = B * W
# the restrictions an entry point may pass: step / step_segments / the merged sequential
# API (none), the sequential two-collective step, a 1-GPU step with a prefetch callback
ENTRIES = [{}, {"allow_csr": False}, {"prefetch": True}]


@pytest.mark.parametrize("args,kw,want", [
    ((B, W, NNZ), {}, "flat"),                                  # plain, supported width
    ((B, W, NNZ), {"width_ok": False}, "compact"),              # no fused instance of the width
    ((B, W, NNZ - 1), {}, "compact"),                           # nnz != B * width
    ((B, None, NNZ), {}, "compact"),                            # no width and no row_ptr
    ((B, W, NNZ), {"vals": True}, "flat_csr"),                  # valued
    ((B, None, NNZ + 7), {"row_ptr": True}, "flat_csr"),        # variable width
    ((B, W, NNZ), {"row_ptr": True, "vals": True, "rows": True}, "flat_csr"),
    ((B, W, NNZ), {"rows": True}, "compact"),                   # rows alone, fixed width
    ((B, W, NNZ), {"vals": True, "allow_csr": False}, "compact"),
    ((B, None, NNZ), {"row_ptr": True, "allow_csr": False}, "compact"),
    ((B, W, NNZ), {"allow_csr": False}, "flat"),                # (restricts CSR only)
    ((B, W, NNZ), {"exchange_ok": False}, "compact"),
    ((B, W, NNZ), {"vals": True, "exchange_ok": False}, "compact"),
    ((B, W, NNZ), {"flat_loc": False}, "compact"),              # a compact localisation
    ((B, W, NNZ), {"vals": True, "flat_loc": False}, "compact"),
    ((B, W, NNZ), {"prefetch": True}, "compact"),               # 1 GPU: the generic step
    ((B, W, NNZ), {"vals": True, "prefetch": True}, "compact"),
    ((_CSR_MAX_ROWS - 1, W, (_CSR_MAX_ROWS - 1) * W), {"vals": True}, "flat_csr"),
    ((_CSR_MAX_ROWS, W, _CSR_MAX_ROWS * W), {}, "flat"),        # (the CSR row limit only)
    (((1 << 25) - 1, 1, (1 << 25) - 1), {}, "flat"),
    ((1 << 25, 1, 1 << 25), {}, "compact"),                     # the flat accumulators' limit
])
def test_route_table(args, kw, want):
    assert route(*args, **kw) == want


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("operands", [{"vals": True}, {"row_ptr": True},
                                      {"row_ptr": True, "vals": True, "rows": True}])
def test_csr_row_limit_goes_compact_from_every_entry_point(entry, operands):
    """tp_fwd_bwd_csr encodes rows in 19 bits: valued or variable-width minibatches of
    _CSR_MAX_ROWS rows or more never reach it."""
    for rows in (_CSR_MAX_ROWS, _CSR_MAX_ROWS + 1):
        assert route(rows, W, rows * W, **operands, **entry) == "compact"


def test_trainer_route_reads_the_localisation(monkeypatch):
    """The trainer's wrapper: a compact ``loc`` (or no flat mode) is compact without
    asking the native library; a flat one goes through ``route``."""
    from types import SimpleNamespace

    tr = SparseLRTrainer(SparseLRConfig(num_features=1 << 20, minibatch=B,
                                        table_capacity=1 << 12))
    assert tr.localize_mode != "tpf"  # (CPU)
    assert tr._route(B, W, NNZ, None, None, None, None) == "compact"
    monkeypatch.setattr(SparseLRTrainer, "_WIDTH_OK", {W: True, 40: False})
    flat, compact = SimpleNamespace(flat=True), SimpleNamespace()
    assert tr._route(B, W, NNZ, None, None, None, flat) == "flat"
    assert tr._route(B, 40, B * 40, None, None, None, flat) == "compact"
    assert tr._route(B, W, NNZ, None, None, object(), flat) == "flat_csr"
    assert tr._route(B, W, NNZ, None, None, object(), flat, allow_csr=False) == "compact"
    assert tr._route(B, W, NNZ, None, None, None, compact) == "compact"
    big = _CSR_MAX_ROWS
    assert tr._route(big, W, big * W, None, None, object(), flat) == "compact"


def test_ssp_apply_is_checked_at_construction():
    with pytest.raises(ValueError, match="ssp_apply"):
        SparseLRTrainer(SparseLRConfig(ssp_apply="sideways"))
