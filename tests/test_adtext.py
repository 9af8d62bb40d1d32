"""The CPU side of the ADFEA / TERAFEA text parser (ops/textparse.py; ops/adtext.py keeps its
earlier names): which formats it claims (and what the one table says of all eight names),
the host route of ``parse_ad_text_device`` (CPU buffers and bytes; the slot ids come from the
host batch), ``SlotReader`` staying on the host route without a GPU, and ``write_text``
writing both formats so that the host parser gives the groups back."""
import numpy as np
import pytest
import torch

from parameter_server_amd import data
from parameter_server_amd.data.slot_reader import SlotReader
from parameter_server_amd.data.synthetic import sparse_groups, write_text
from parameter_server_amd.ops import adtext, pstext, textparse

RAW = {
    "ADFEA": (b"99 1 1 10:1 20:2 18446744073709551615:7\n7 1 0 30:1\n8 1 -3\n"
              b"5 1 x 3:4\n9\t1\t+1\t5:6\r\n"),
    "TERAFEA": (b"1 55 | 18014398509481985 5 18446744073709551615\n0 56 | 7\n-2 57 |\n"
                b"x 1 | 3\n+1\t58\t|\t36028797018963970\r\n"),
}
NAMES = ("DENSE", "SPARSE", "SPARSE_BINARY", "ADFEA", "LIBSVM", "TERAFEA", "VW", "CRITEO")


def test_supported_formats():
    assert [data.TEXT_FORMATS[f] for f in NAMES] == list(range(1, 9))
    for f in ("ADFEA", "TERAFEA", 4, 6):
        assert adtext.supported(f)
        assert textparse.supported(f) and textparse.produces_slots(f)
        assert textparse.traits(f).family == "adtext" and not textparse.traits(f).valued
    # the one table, by name and by id: every format but DENSE and VW, each in its family
    family = {"LIBSVM": "textparse", "CRITEO": "textparse", "SPARSE": "pstext",
              "SPARSE_BINARY": "pstext", "ADFEA": "adtext", "TERAFEA": "adtext"}
    for k, f in enumerate(NAMES, 1):
        assert textparse.supported(f) == textparse.supported(k) == (f in family)
        t = textparse.traits(f)
        assert t == textparse.traits(k) and (t.family if t else None) == family.get(f)
        assert t is None or t.id == k
        # the family modules claim what they claimed
        assert adtext.supported(f) == adtext.supported(k) == (f in ("ADFEA", "TERAFEA"))
        assert pstext.supported(f) == pstext.supported(k) == (f in ("SPARSE", "SPARSE_BINARY"))


@pytest.mark.parametrize("ignore_slot", [True, False])
@pytest.mark.parametrize("fmt", ["ADFEA", "TERAFEA"])
@pytest.mark.parametrize("as_bytes", [True, False])
def test_cpu_buffers_take_the_host_parser(fmt, ignore_slot, as_bytes):
    raw = RAW[fmt]
    ref = data.parse_text(raw, fmt, ignore_slot=ignore_slot, hash_mod=1000)
    buf = raw if as_bytes else torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    got = adtext.parse_ad_text_device(buf, fmt, 1000, ignore_slot=ignore_slot)
    assert got.deferred is False and not got.keys.is_cuda
    assert (got.rows, got.nnz) == (ref.rows, ref.nnz) and got.rows == 4
    assert got.bad_lines == ref.info["bad_lines"] == 1
    assert np.array_equal(got.labels.numpy(), ref.labels)
    assert np.array_equal(got.row_ptr.numpy(), ref.row_ptr)
    assert np.array_equal(got.keys.numpy().view(np.uint64), ref.keys)
    assert got.vals is None and ref.vals is None
    if ignore_slot:
        assert got.slots is None
    else:
        assert got.slots.dtype == torch.int32
        assert np.array_equal(got.slots.numpy(), ref.slots)
        assert len(set(ref.slots.tolist())) >= 3


@pytest.mark.parametrize("fmt", ["ADFEA", "TERAFEA"])
def test_cpu_route_behind_carried_rows_keeps_slots(fmt):
    first = RAW[fmt].split(b"\n")[1] + b"\n"
    out = textparse.TextParseBuffers(4, 8, "cpu")
    a = adtext.parse_ad_text_device(first, fmt, ignore_slot=False, out=out)
    b = adtext.parse_ad_text_device(RAW[fmt], fmt, ignore_slot=False, out=out, row0=a.rows,
                                    nnz0=a.nnz)
    ref = data.parse_text(first + RAW[fmt], fmt, ignore_slot=False)
    n = a.nnz + b.nnz
    assert (a.rows + b.rows, n) == (ref.rows, ref.nnz) and a.rows == 1
    assert np.array_equal(out.slots[:n].numpy(), ref.slots)  # (grown and carried like keys)
    assert np.array_equal(out.keys[:n].numpy().view(np.uint64), ref.keys)
    assert np.array_equal(out.row_ptr[:ref.rows + 1].numpy(), ref.row_ptr)
    assert np.array_equal(out.labels[:ref.rows].numpy(), ref.labels)


def test_unknown_format_raises_on_no_route():
    with pytest.raises(KeyError):
        adtext.parse_ad_text_device(b"1 2 3\n", "NOPE")


def _same(a, b):
    assert np.array_equal(a.labels, b.labels) and sorted(a.groups) == sorted(b.groups)
    for g in a.groups:
        for u, v in zip(a.groups[g], b.groups[g]):
            assert (u is None) == (v is None)
            if u is not None:
                assert u.dtype == v.dtype and np.array_equal(u, v)


def test_slot_reader_without_a_gpu_stays_on_the_host(tmp_path):
    p = tmp_path / "part-0"
    p.write_bytes(RAW["ADFEA"])
    ref = SlotReader([str(p)], "ADFEA").read()
    assert sorted(ref.groups) == [1, 2, 6, 7]
    for device in ("cpu", None):
        for split in ("host", "device"):
            r = SlotReader([str(p)], "ADFEA", parser="gpu", device=device, split=split)
            assert r.parser == "cpu" and r.split == "host"
            _same(r.read(), ref)


@pytest.mark.parametrize("fmt", ["ADFEA", "TERAFEA"])
def test_write_text_round_trip(tmp_path, fmt):
    sd = sparse_groups(300, groups=5, present=3, keys_per_group=500, seed=3)
    assert len(sd.groups) == 5 and any((np.diff(o) == 0).any() for o, _, _ in sd.groups.values())
    path = str(tmp_path / "part-0")
    write_text(sd, path, fmt)
    first = open(path).readline().split()
    assert first[:2] == ["0", "1"] if fmt == "ADFEA" else first[1:3] == ["0", "|"]
    back = SlotReader([path], fmt).read()
    assert np.array_equal(back.labels, np.where(sd.labels > 0, 1, -1).astype(np.float32))
    assert sorted(back.groups) == sorted(sd.groups)
    for g, (off, keys, vals) in sd.groups.items():
        boff, bkeys, bvals = back.groups[g]
        assert bvals is None and np.array_equal(boff, off)
        # TERAFEA keeps the group in the key's top 10 bits and 54 bits of the key
        want = keys.astype(np.uint64) if fmt == "ADFEA" else \
            (np.uint64(g) << np.uint64(54)) | (keys.astype(np.uint64) & np.uint64((1 << 54) - 1))
        assert np.array_equal(bkeys, want)
    # the existing formats are written as before
    write_text(sd, path, "SPARSE_BINARY")
    _same(SlotReader([path], "SPARSE_BINARY").read(), SlotReader([path], "SPARSE_BINARY").read())
    assert open(path).readline().count(";") >= 1
