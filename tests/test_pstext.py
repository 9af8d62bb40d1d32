"""The CPU side of the slot-grouped text parser (ops/textparse.py; ops/pstext.py keeps its
earlier names): which formats it claims, the host route of ``parse_ps_text_device`` (CPU
buffers and bytes; the slot ids come from the host batch), and ``SlotReader`` staying on the
host route without a GPU."""
import numpy as np
import pytest
import torch

from parameter_server_amd import data
from parameter_server_amd.data.slot_reader import SlotReader
from parameter_server_amd.ops import pstext, textparse

RAW = (b"1; 3 5 6 18446744073709551615; 7 9\n0;2 4;\n-1; 4096 1;; 3 2\n"
       b"x; 1 2\n+1; 5 7\r\n")
RAW_V = b"1; 3 5:0.5 6:1; 7 9:-2e-3\n0; 2 4:1\n"


def test_supported_formats():
    for f in ("SPARSE_BINARY", "SPARSE", 2, 3):
        assert pstext.supported(f)
        assert textparse.supported(f) and textparse.produces_slots(f)
        assert textparse.traits(f).family == "pstext"
    for f in ("LIBSVM", "CRITEO", "DENSE", "ADFEA", "TERAFEA", "VW", 1, 4, 5, 6, 7, 8):
        assert not pstext.supported(f)
    assert textparse.traits("SPARSE").valued and not textparse.traits("SPARSE_BINARY").valued
    # the one entry claims the six formats with kernels, and no other
    for f in ("LIBSVM", "CRITEO", "ADFEA", "TERAFEA", 4, 5, 6, 8):
        assert textparse.supported(f) and textparse.traits(f).family != "pstext"
    for f in ("DENSE", "VW", 1, 7):
        assert not textparse.supported(f) and not textparse.produces_slots(f)
    # LIBSVM / CRITEO have no slot ids to keep
    for f in ("LIBSVM", "CRITEO"):
        assert not textparse.produces_slots(f)
        with pytest.raises(ValueError):
            textparse.parse_text_device(b"1 2:3\n", f, ignore_slot=False)


@pytest.mark.parametrize("ignore_slot", [True, False])
@pytest.mark.parametrize("fmt,raw", [("SPARSE_BINARY", RAW), ("SPARSE", RAW_V)])
@pytest.mark.parametrize("as_bytes", [True, False])
def test_cpu_buffers_take_the_host_parser(fmt, raw, ignore_slot, as_bytes):
    ref = data.parse_text(raw, fmt, ignore_slot=ignore_slot, hash_mod=1000)
    buf = raw if as_bytes else torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    got = pstext.parse_ps_text_device(buf, fmt, 1000, ignore_slot=ignore_slot)
    assert got.deferred is False and not got.keys.is_cuda
    assert (got.rows, got.nnz) == (ref.rows, ref.nnz) and got.rows >= 2
    assert got.bad_lines == ref.info["bad_lines"]
    assert np.array_equal(got.labels.numpy(), ref.labels)
    assert np.array_equal(got.row_ptr.numpy(), ref.row_ptr)
    assert np.array_equal(got.keys.numpy().view(np.uint64), ref.keys)
    assert (got.vals is None) == (ref.vals is None)
    if ref.vals is not None:
        assert np.array_equal(got.vals.numpy(), ref.vals)
    if ignore_slot:
        assert got.slots is None
    else:
        assert got.slots.dtype == torch.int32
        assert np.array_equal(got.slots.numpy(), ref.slots)


def test_cpu_route_behind_carried_rows_keeps_slots():
    out = textparse.TextParseBuffers(4, 8, "cpu")
    a = pstext.parse_ps_text_device(b"1; 3 5 6\n", "SPARSE_BINARY", ignore_slot=False, out=out)
    b = pstext.parse_ps_text_device(RAW, "SPARSE_BINARY", ignore_slot=False, out=out,
                                    row0=a.rows, nnz0=a.nnz)
    ref = data.parse_text(b"1; 3 5 6\n" + RAW, "SPARSE_BINARY", ignore_slot=False)
    n = a.nnz + b.nnz
    assert (a.rows + b.rows, n) == (ref.rows, ref.nnz)
    assert np.array_equal(out.slots[:n].numpy(), ref.slots)  # (grown and carried like keys)
    assert np.array_equal(out.keys[:n].numpy().view(np.uint64), ref.keys)
    assert np.array_equal(out.row_ptr[:ref.rows + 1].numpy(), ref.row_ptr)


def test_unknown_format_raises_on_no_route():
    with pytest.raises(KeyError):
        pstext.parse_ps_text_device(b"1; 2 3\n", "NOPE")


def test_slot_reader_without_a_gpu_stays_on_the_host(tmp_path):
    p = tmp_path / "part-0"
    p.write_bytes(RAW)
    ref = SlotReader([str(p)], "SPARSE_BINARY").read()
    for device in ("cpu", None):
        r = SlotReader([str(p)], "SPARSE_BINARY", parser="gpu", device=device)
        assert r.parser == "cpu"
        got = r.read()
        assert np.array_equal(got.labels, ref.labels) and sorted(got.groups) == sorted(ref.groups)
        for g in ref.groups:
            assert np.array_equal(got.groups[g][0], ref.groups[g][0])
            assert np.array_equal(got.groups[g][1], ref.groups[g][1])
    with pytest.raises(ValueError):
        SlotReader([str(p)], "SPARSE_BINARY", parser="fast")
