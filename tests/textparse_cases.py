"""What the GPU tests of the device text parsers (test_textparse_gpu.py, test_pstext_gpu.py,
test_adtext_gpu.py) share: the upload of a text and the comparison of ``parse_text_device``
with the host parser on the same bytes."""
import numpy as np
import torch

from parameter_server_amd import data
from parameter_server_amd.ops.textparse import parse_text_device, traits

DEV = "cuda"
SPAN = 16384  # bytes of text per workgroup (textparse.cuh)


def _dev(raw: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV) if raw else \
        torch.empty(0, dtype=torch.uint8, device=DEV)


def check_against_host(raw: bytes, fmt: str, hash_mod: int = 0, *, ignore_slot: bool,
                       clean: bool = True, out=None):
    """Device result == host result on ``raw``; returns the device result."""
    ref = data.parse_text(raw, fmt, ignore_slot=ignore_slot, hash_mod=hash_mod)
    got = parse_text_device(_dev(raw), fmt, hash_mod, ignore_slot=ignore_slot, out=out)
    torch.cuda.synchronize()
    assert got.rows == ref.rows and got.nnz == ref.nnz
    assert got.bad_lines == ref.info["bad_lines"]
    assert np.array_equal(got.labels.cpu().numpy().view(np.uint32),
                          np.asarray(ref.labels, np.float32).view(np.uint32))
    assert np.array_equal(got.row_ptr.cpu().numpy(), np.asarray(ref.row_ptr, np.int64))
    assert np.array_equal(got.keys.cpu().numpy().view(np.uint64),
                          np.asarray(ref.keys).view(np.uint64))
    assert (got.vals is None) == (ref.vals is None)
    if ref.vals is not None:
        assert traits(fmt).valued
        assert np.array_equal(got.vals.cpu().numpy().view(np.uint32),
                              np.asarray(ref.vals, np.float32).view(np.uint32))
    if ignore_slot:
        assert got.slots is None
    else:
        assert got.slots.dtype == torch.int32
        assert np.array_equal(got.slots.cpu().numpy(), np.asarray(ref.slots, np.int32))
    w = np.diff(np.asarray(ref.row_ptr))
    assert got.width == (int(w[0]) if w.size and w[0] > 0 and (w == w[0]).all() else 0)
    if clean:
        assert got.deferred is False and ref.info["bad_lines"] == 0
    assert int(got.out.hdr.cpu()[7]) == 0  # capacity flag clear
    return got
