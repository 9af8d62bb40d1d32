// Bindings of the data-preparation kernels: generic localisation (localize.hip,
// primitives.hip, sort32.hip, partloc.hip), the filters (filters.hip) and the text
// parsers / formatter (textparse.hip, pstext.hip, adtext.hip, modeltext.hip).
#include "bind_common.h"
#include "filters.h"
#include "localize.h"
#include "modeltext.h"
#include "partloc.h"
#include "primitives.h"
#include "sort32.h"
#include "textparse.h"

using namespace psamd_bind;

namespace {

// the two optional n-float buffers a localiser clears in its pass
struct ZeroPair {
  float *a, *b;
};
ZeroPair zero_pair(const optional<Tensor>& zero_a, const optional<Tensor>& zero_b, int64_t n) {
  float* za = optr<float>(zero_a, at::kFloat, "zero_a");
  float* zb = optr<float>(zero_b, at::kFloat, "zero_b");
  if (za) check(zero_a->numel() >= n, "zero_a too small");
  if (zb) check(zero_b->numel() >= n, "zero_b too small");
  return {za, zb};
}

// CountMin over byte cells packed in int32 words: one region of all cells, or (rshift
// < 64) regions of rsize cells selected by key >> rshift (countmin.cuh)
uint64_t cm_rsize(const Tensor& table, int64_t rsize, int rshift, int key_bits) {
  const uint64_t n = (uint64_t)table.numel() * 4;
  if (rshift >= 64) return rsize > 0 ? std::min<uint64_t>((uint64_t)rsize, n) : n;
  check(rsize > 0 && rsize % 64 == 0,
        "countmin: region size must be a positive multiple of 64 (one block)");
  check(rshift >= 0 && key_bits >= rshift && key_bits - rshift <= 30 &&
            ((uint64_t)rsize << (key_bits - rshift)) <= n,
        "countmin: regions exceed the cell table");
  return (uint64_t)rsize;
}

}  // namespace

void psamd_bind::register_prep(py::module_& m) {
  // ---------------- text parsing ----------------
  m.def("textparse_work_words", [](int64_t n, int fmt) {
    return psamd::textparse_work_words(n, fmt);
  }, py::arg("n"), py::arg("fmt") = psamd::kFmtLibsvm);
  m.def("textparse", [](Tensor text, int64_t n, int fmt, uint64_t hash_mod, int64_t row0,
                        int64_t nnz0, Tensor labels, Tensor row_ptr, Tensor keys,
                        optional<Tensor> vals, optional<Tensor> slots, Tensor hdr, Tensor work) {
    chk(text, at::kByte, "text");
    chk(labels, at::kFloat, "labels");
    chk(row_ptr, at::kLong, "row_ptr");
    chk(keys, at::kLong, "keys");
    chk(hdr, at::kInt, "hdr");
    chk(work, at::kInt, "work");
    float* vp = optr<float>(vals, at::kFloat, "vals");
    int32_t* sp = optr<int32_t>(slots, at::kInt, "slots");
    check(n >= 1 && n <= text.numel(), "textparse: n outside the text buffer");
    check(row0 >= 0 && nnz0 >= 0 && row0 < row_ptr.numel(), "textparse: bad base offsets");
    check(hdr.numel() >= 8, "textparse: header needs 8 words");
    check(work.numel() >= psamd::textparse_work_words(n, fmt), "textparse: work buffer too small");
    int64_t cap_nnz = keys.numel();
    if (vp) cap_nnz = std::min<int64_t>(cap_nnz, vals->numel());
    if (sp) cap_nnz = std::min<int64_t>(cap_nnz, slots->numel());
    psamd::textparse(ptr<uint8_t>(text), n, fmt, hash_mod,
                     {ptr<float>(labels), labels.numel(), ptr<int64_t>(row_ptr), row_ptr.numel(),
                      ptr<uint64_t>(keys), vp, sp, cap_nnz, row0, nnz0, ptr<int32_t>(hdr)},
                     ptr<int32_t>(work), cur_stream());
  }, py::arg("text"), py::arg("n"), py::arg("fmt"), py::arg("hash_mod"), py::arg("row0"),
     py::arg("nnz0"), py::arg("labels"), py::arg("row_ptr"), py::arg("keys"), py::arg("vals"),
     py::arg("slots"), py::arg("hdr"), py::arg("work"));
  m.def("textparse_rebase", [](Tensor in, Tensor out, int64_t n, int64_t delta) {
    chk(in, at::kLong, "in");
    chk(out, at::kLong, "out");
    check(n >= 0 && in.numel() >= n && out.numel() >= n, "textparse_rebase: buffers too small");
    psamd::textparse_rebase(ptr<int64_t>(in), ptr<int64_t>(out), n, delta, cur_stream());
  });
  m.def("textparse_seg_nonunit", [](Tensor vals, Tensor bounds, Tensor flags) {
    chk(vals, at::kFloat, "vals");
    chk(bounds, at::kLong, "bounds");
    chk(flags, at::kInt, "flags");
    const int64_t nseg = bounds.numel() - 1;
    check(nseg >= 0 && nseg < (1 << 30) && flags.numel() >= nseg,
          "textparse_seg_nonunit: flags too small");
    psamd::textparse_seg_nonunit(ptr<float>(vals), vals.numel(), ptr<int64_t>(bounds), (int)nseg,
                                 ptr<int32_t>(flags), cur_stream());
  });

  // ---------------- model text ----------------
  m.def("modeltext_block", [] { return psamd::modeltext_block(); });
  m.def("modeltext_max_entry", [] { return psamd::modeltext_max_entry(); });
  m.def("modeltext_work_bytes", [](int64_t n) { return psamd::modeltext_work_bytes(n); });
  m.def("modeltext_format", [](Tensor keys, Tensor w, Tensor out, Tensor hdr, Tensor work) {
    chk(keys, at::kLong, "keys");
    chk(w, at::kFloat, "w");
    chk(out, at::kByte, "out");
    chk(hdr, at::kLong, "hdr");
    chk(work, at::kByte, "work");
    const int64_t n = keys.numel();
    check(n >= 1 && w.numel() == n, "modeltext_format: keys and w must be equally long, not empty");
    check(out.numel() >= n * psamd::modeltext_max_entry(), "modeltext_format: out too small");
    check(hdr.numel() >= 3, "modeltext_format: header needs 3 words");
    check(work.numel() >= psamd::modeltext_work_bytes(n), "modeltext_format: work buffer too small");
    psamd::modeltext_format(ptr<uint64_t>(keys), reinterpret_cast<const uint32_t*>(ptr<float>(w)), n,
                            ptr<uint8_t>(out), out.numel(), ptr<int64_t>(hdr), ptr<uint8_t>(work),
                            cur_stream());
  }, py::arg("keys"), py::arg("w"), py::arg("out"), py::arg("hdr"), py::arg("work"));
  m.def("modeltext_parse", [](Tensor text, int64_t n, Tensor keys, Tensor w, Tensor hdr,
                              Tensor work) {
    chk(text, at::kByte, "text");
    chk(keys, at::kLong, "keys");
    chk(w, at::kFloat, "w");
    chk(hdr, at::kInt, "hdr");
    chk(work, at::kInt, "work");
    check(n >= 1 && n <= text.numel(), "modeltext_parse: n outside the text buffer");
    check(hdr.numel() >= 8, "modeltext_parse: header needs 8 words");
    check(work.numel() >= psamd::textparse_work_words(n), "modeltext_parse: work buffer too small");
    const int64_t cap = std::min<int64_t>(keys.numel(), w.numel());
    check(cap >= 1, "modeltext_parse: empty outputs");
    psamd::modeltext_parse(ptr<uint8_t>(text), n, ptr<uint64_t>(keys), ptr<float>(w), cap,
                           ptr<int32_t>(hdr), ptr<int32_t>(work), cur_stream());
  }, py::arg("text"), py::arg("n"), py::arg("keys"), py::arg("w"), py::arg("hdr"), py::arg("work"));

  // ---------------- localisation ----------------
  m.def("mix_iota", [](Tensor keys, int bits, Tensor h, Tensor pos) {
    chk(keys, at::kLong, "keys");
    chk(h, at::kLong, "h");
    chk(pos, at::kInt, "pos");
    const int64_t n = keys.numel();
    check(h.numel() >= n && pos.numel() >= n, "outputs too small");
    psamd::mix_iota(ptr<uint64_t>(keys), n, make_keymix(bits), ptr<uint64_t>(h), ptr<int32_t>(pos),
                    cur_stream());
  });
  m.def("mix_keys", [](Tensor keys, int bits, Tensor out, bool inverse) {
    chk(keys, at::kLong, "keys");
    chk(out, at::kLong, "out");
    check(out.numel() >= keys.numel(), "out too small");
    psamd::mix_keys(ptr<uint64_t>(keys), keys.numel(), make_keymix(bits), ptr<uint64_t>(out),
                    inverse, cur_stream());
  });
  m.def("sort_pairs_temp_bytes", [](int64_t n, int /*end_bit*/) {
    return (int64_t)psamd::radix_sort_temp_bytes(n);
  }, py::arg("n"), py::arg("end_bit"));
  m.def("sort_pairs", [](Tensor temp, Tensor k_in, Tensor k_out, Tensor v_in, Tensor v_out,
                         int64_t n, int end_bit) {
    chk(temp, at::kByte, "temp");
    chk(k_in, at::kLong, "k_in");
    chk(k_out, at::kLong, "k_out");
    chk(v_in, at::kInt, "v_in");
    chk(v_out, at::kInt, "v_out");
    check(n >= 0 && k_in.numel() >= n && k_out.numel() >= n && v_in.numel() >= n &&
              v_out.numel() >= n, "sort buffers too small");
    check(n < (int64_t)INT32_MAX, "sort size must fit int32");
    check(end_bit >= 1 && end_bit <= 64, "end_bit in [1,64]");
    check(k_in.data_ptr() != k_out.data_ptr() && v_in.data_ptr() != v_out.data_ptr(),
          "sort input and output must not alias");
    check((size_t)temp.numel() >= psamd::radix_sort_temp_bytes(n),
          "sort temp storage too small");
    psamd::radix_sort_pairs(temp.data_ptr(), (size_t)temp.numel(), ptr<uint64_t>(k_in),
                            ptr<uint64_t>(k_out), ptr<int32_t>(v_in), ptr<int32_t>(v_out), n,
                            end_bit, cur_stream());
  }, py::arg("temp"), py::arg("k_in"), py::arg("k_out"), py::arg("v_in"), py::arg("v_out"),
     py::arg("n"), py::arg("end_bit"));
  m.def("scan_temp_bytes", [](int64_t n) { return (int64_t)psamd::scan_temp_bytes(n); });
  m.def("inclusive_scan_i32", [](Tensor temp, Tensor in, Tensor out, int64_t n) {
    chk(temp, at::kByte, "temp");
    chk(in, at::kInt, "in");
    chk(out, at::kInt, "out");
    check(in.numel() >= n && out.numel() >= n, "scan buffers too small");
    check((size_t)temp.numel() >= psamd::scan_temp_bytes(n), "scan temp too small");
    psamd::inclusive_scan_i32(temp.data_ptr(), (size_t)temp.numel(), ptr<int32_t>(in),
                              ptr<int32_t>(out), n, cur_stream());
  });
  m.def("rle", [](Tensor hs, Tensor pos_s, int64_t n, Tensor flags, Tensor segid, Tensor scan_temp,
                  Tensor uniq, Tensor seg_start, Tensor local_col, Tensor n_uniq,
                  optional<Tensor> zero_a, optional<Tensor> zero_b) {
    chk(hs, at::kLong, "hs");
    chk(pos_s, at::kInt, "pos_s");
    chk(flags, at::kInt, "flags");
    chk(segid, at::kInt, "segid");
    chk(scan_temp, at::kByte, "scan_temp");
    chk(uniq, at::kLong, "uniq");
    chk(seg_start, at::kInt, "seg_start");
    chk(local_col, at::kInt, "local_col");
    chk(n_uniq, at::kInt, "n_uniq");
    check(n >= 1, "rle needs n >= 1");
    check(hs.numel() >= n && pos_s.numel() >= n && flags.numel() >= n && segid.numel() >= n &&
              uniq.numel() >= n && seg_start.numel() >= n + 1 && local_col.numel() >= n,
          "rle buffers too small");
    const ZeroPair z = zero_pair(zero_a, zero_b, n);
    check((size_t)scan_temp.numel() >= psamd::scan_temp_bytes(n), "scan temp too small");
    psamd::rle(ptr<uint64_t>(hs), ptr<int32_t>(pos_s), n, ptr<int32_t>(flags), ptr<int32_t>(segid),
               scan_temp.data_ptr(), (size_t)scan_temp.numel(), ptr<uint64_t>(uniq),
               ptr<int32_t>(seg_start), ptr<int32_t>(local_col), ptr<int32_t>(n_uniq), z.a, z.b,
               cur_stream());
  });
  m.def("localize32_temp_bytes", [](int64_t n) { return (int64_t)psamd::localize32_temp_bytes(n); });
  m.def("sort40_temp_bytes", [](int64_t n) { return (int64_t)psamd::sort40_temp_bytes(n); });
  m.def("sort40", [](Tensor keys, int bits, Tensor temp, Tensor hs, Tensor pos_s) {
    chk(keys, at::kLong, "keys");
    chk(temp, at::kByte, "temp");
    chk(hs, at::kLong, "hs");
    chk(pos_s, at::kInt, "pos_s");
    const int64_t n = keys.numel();
    check(n >= 1 && n < (int64_t(1) << 22), "sort40: 1 <= n < 2^22");
    check(bits > 30 && bits <= 40, "sort40 needs 30 < key bits <= 40");
    check(hs.numel() >= n && pos_s.numel() >= n, "sort40 buffers too small");
    check((size_t)temp.numel() >= psamd::sort40_temp_bytes(n), "sort40 temp too small");
    psamd::sort40(ptr<uint64_t>(keys), n, make_keymix(bits), temp.data_ptr(),
                  (size_t)temp.numel(), ptr<uint64_t>(hs), ptr<int32_t>(pos_s), cur_stream());
  });
  m.def("localize32", [](Tensor keys, int bits, Tensor temp, Tensor hs, Tensor pos_s, Tensor segid,
                         Tensor uniq, Tensor seg_start, Tensor local_col, Tensor n_uniq,
                         optional<Tensor> zero_a, optional<Tensor> zero_b, int digit_bits) {
    check(digit_bits == 8 || digit_bits == 10, "localize32 digit_bits: 8 or 10");
    chk(keys, at::kLong, "keys");
    chk(temp, at::kByte, "temp");
    chk(hs, at::kInt, "hs");
    chk(pos_s, at::kInt, "pos_s");
    chk(segid, at::kInt, "segid");
    chk(uniq, at::kLong, "uniq");
    chk(seg_start, at::kInt, "seg_start");
    chk(local_col, at::kInt, "local_col");
    chk(n_uniq, at::kInt, "n_uniq");
    const int64_t n = keys.numel();
    check(n >= 1 && n < (int64_t)INT32_MAX, "localize32: 1 <= n < 2^31");
    check(bits >= 2 && bits <= 32, "localize32 needs key bits <= 32");
    check(hs.numel() >= n && pos_s.numel() >= n && segid.numel() >= n && uniq.numel() >= n &&
              seg_start.numel() >= n + 1 && local_col.numel() >= n, "localize32 buffers too small");
    check((size_t)temp.numel() >= psamd::localize32_temp_bytes(n), "localize32 temp too small");
    const ZeroPair z = zero_pair(zero_a, zero_b, n);
    psamd::localize32(ptr<uint64_t>(keys), n, make_keymix(bits), temp.data_ptr(),
                      (size_t)temp.numel(), ptr<uint32_t>(hs), ptr<int32_t>(pos_s),
                      ptr<int32_t>(segid), ptr<uint64_t>(uniq), ptr<int32_t>(seg_start),
                      ptr<int32_t>(local_col), ptr<int32_t>(n_uniq), z.a, z.b, digit_bits,
                      cur_stream());
  }, py::arg("keys"), py::arg("bits"), py::arg("temp"), py::arg("hs"), py::arg("pos_s"),
     py::arg("segid"), py::arg("uniq"), py::arg("seg_start"), py::arg("local_col"),
     py::arg("n_uniq"), py::arg("zero_a"), py::arg("zero_b"), py::arg("digit_bits") = 8);
  m.def("partloc_temp_bytes", [](int64_t n, int bits) {
    return (int64_t)psamd::partloc_temp_bytes(n, bits);
  });
  m.def("partloc_supported", [](int64_t n, int bits) { return psamd::partloc_supported(n, bits); });
  m.def("localize_part", [](Tensor keys, int bits, Tensor temp, Tensor pos_s, Tensor segid,
                            Tensor uniq, Tensor seg_start, Tensor local_col, Tensor n_uniq,
                            optional<Tensor> zero_a, optional<Tensor> zero_b, Tensor err) {
    chk(keys, at::kLong, "keys");
    chk(temp, at::kByte, "temp");
    chk(pos_s, at::kInt, "pos_s");
    chk(segid, at::kInt, "segid");
    chk(uniq, at::kLong, "uniq");
    chk(seg_start, at::kInt, "seg_start");
    chk(local_col, at::kInt, "local_col");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(err, at::kInt, "err");
    const int64_t n = keys.numel();
    check(psamd::partloc_supported(n, bits), "localize_part: needs bits <= 32 and n <= 10M");
    check(pos_s.numel() >= n && segid.numel() >= n && uniq.numel() >= n &&
              seg_start.numel() >= n + 1 && local_col.numel() >= n,
          "localize_part buffers too small");
    check((size_t)temp.numel() >= psamd::partloc_temp_bytes(n, bits), "localize_part temp too small");
    const ZeroPair z = zero_pair(zero_a, zero_b, n);
    psamd::localize_part(ptr<uint64_t>(keys), n, make_keymix(bits), temp.data_ptr(),
                         (size_t)temp.numel(), ptr<int32_t>(pos_s), ptr<int32_t>(segid),
                         ptr<uint64_t>(uniq), ptr<int32_t>(seg_start), ptr<int32_t>(local_col),
                         ptr<int32_t>(n_uniq), z.a, z.b, ptr<int32_t>(err), uniq.numel(),
                         cur_stream());
  });
  m.def("owner_split", [](Tensor uniq, optional<Tensor> n_uniq, Tensor bounds, Tensor offsets) {
    chk(uniq, at::kLong, "uniq");
    chk(bounds, at::kLong, "bounds");
    chk(offsets, at::kLong, "offsets");
    const int G = (int)bounds.numel() - 1;
    check(G >= 1 && offsets.numel() >= G + 1, "bounds/offsets size mismatch");
    psamd::owner_split(ptr<uint64_t>(uniq), optr<int32_t>(n_uniq, at::kInt, "n_uniq"),
                       uniq.numel(), ptr<uint64_t>(bounds), G, ptr<int64_t>(offsets),
                       cur_stream());
  });
  m.def("owner_of", [](Tensor h, Tensor bounds, Tensor owner) {
    chk(h, at::kLong, "h");
    chk(bounds, at::kLong, "bounds");
    chk(owner, at::kInt, "owner");
    const int G = (int)bounds.numel() - 1;
    check(G >= 1 && owner.numel() >= h.numel(), "owner_of sizes");
    psamd::owner_of(ptr<uint64_t>(h), h.numel(), ptr<uint64_t>(bounds), G, ptr<int32_t>(owner),
                    cur_stream());
  });

  // ---------------- filters ----------------
  m.def("cm_insert", [](Tensor table, int k, int vmax, Tensor keys, optional<Tensor> counts,
                        optional<Tensor> n_dev, int64_t rsize, int rshift, int key_bits) {
    chk(table, at::kInt, "table");
    chk(keys, at::kLong, "keys");
    check(k >= 1 && k <= 30 && vmax >= 1 && vmax <= 255, "countmin k/vmax");
    const uint8_t* c = optr<uint8_t>(counts, at::kByte, "counts");
    if (c) check(counts->numel() >= keys.numel(), "counts too small");
    psamd::cm_insert(ptr<uint32_t>(table), cm_rsize(table, rsize, rshift, key_bits), rshift, k,
                     (uint32_t)vmax, ptr<uint64_t>(keys), c, keys.numel(),
                     optr<int32_t>(n_dev, at::kInt, "n_dev"), cur_stream());
  }, py::arg("table"), py::arg("k"), py::arg("vmax"), py::arg("keys"), py::arg("counts"),
     py::arg("n_dev"), py::arg("rsize") = 0, py::arg("rshift") = 64, py::arg("key_bits") = 64);
  m.def("cm_query", [](Tensor table, int k, int vmax, Tensor keys, optional<Tensor> n_dev,
                       int freq, optional<Tensor> keep, optional<Tensor> out_count,
                       int64_t rsize, int rshift, int key_bits) {
    chk(table, at::kInt, "table");
    chk(keys, at::kLong, "keys");
    int32_t* kp = optr<int32_t>(keep, at::kInt, "keep");
    uint8_t* cp = optr<uint8_t>(out_count, at::kByte, "out_count");
    if (kp) check(keep->numel() >= keys.numel(), "keep too small");
    if (cp) check(out_count->numel() >= keys.numel(), "out_count too small");
    psamd::cm_query(ptr<uint32_t>(table), cm_rsize(table, rsize, rshift, key_bits), rshift, k,
                    (uint32_t)vmax, ptr<uint64_t>(keys), keys.numel(),
                    optr<int32_t>(n_dev, at::kInt, "n_dev"), freq, kp, cp, cur_stream());
  }, py::arg("table"), py::arg("k"), py::arg("vmax"), py::arg("keys"), py::arg("n_dev"),
     py::arg("freq"), py::arg("keep"), py::arg("out_count"), py::arg("rsize") = 0,
     py::arg("rshift") = 64, py::arg("key_bits") = 64);
  m.def("compact_kept", [](Tensor keep, Tensor incl, optional<Tensor> n_dev, Tensor kept_idx,
                           Tensor n_kept, optional<Tensor> remap, optional<Tensor> keys_in,
                           optional<Tensor> keys_out) {
    chk(keep, at::kInt, "keep");
    chk(incl, at::kInt, "incl");
    chk(kept_idx, at::kInt, "kept_idx");
    chk(n_kept, at::kInt, "n_kept");
    check(kept_idx.numel() >= keep.numel() && incl.numel() >= keep.numel(), "compact sizes");
    const uint64_t* ki = optr<uint64_t>(keys_in, at::kLong, "keys_in");
    uint64_t* ko = optr<uint64_t>(keys_out, at::kLong, "keys_out");
    check((ki == nullptr) == (ko == nullptr), "keys_in and keys_out go together");
    if (ki) check(keys_in->numel() >= keep.numel() && keys_out->numel() >= keep.numel(),
                  "compact key buffers too small");
    psamd::compact_kept(ptr<int32_t>(keep), ptr<int32_t>(incl), keep.numel(),
                        optr<int32_t>(n_dev, at::kInt, "n_dev"), ptr<int32_t>(kept_idx),
                        ptr<int32_t>(n_kept), optr<int32_t>(remap, at::kInt, "remap"), ki, ko,
                        cur_stream());
  });
  m.def("cm_insert_seg", [](Tensor table, int k, int vmax, Tensor keys, Tensor seg_start,
                            optional<Tensor> n_dev, int64_t rsize, int rshift, int key_bits) {
    chk(table, at::kInt, "table");
    chk(keys, at::kLong, "keys");
    chk(seg_start, at::kInt, "seg_start");
    check(k >= 1 && k <= 30 && vmax >= 1 && vmax <= 255, "countmin k/vmax");
    check(seg_start.numel() >= keys.numel() + 1 || n_dev.has_value(), "seg_start too small");
    const int64_t n = std::min<int64_t>(keys.numel(), seg_start.numel() - 1);
    psamd::cm_insert_seg(ptr<uint32_t>(table), cm_rsize(table, rsize, rshift, key_bits), rshift,
                         k, (uint32_t)vmax, ptr<uint64_t>(keys), ptr<int32_t>(seg_start), n,
                         optr<int32_t>(n_dev, at::kInt, "n_dev"), cur_stream());
  }, py::arg("table"), py::arg("k"), py::arg("vmax"), py::arg("keys"), py::arg("seg_start"),
     py::arg("n_dev"), py::arg("rsize") = 0, py::arg("rshift") = 64, py::arg("key_bits") = 64);
  m.def("ff_minmax", [](Tensor x, Tensor mm) {
    chk(x, at::kFloat, "x");
    chk(mm, at::kFloat, "mm");
    check(mm.numel() >= 2, "mm needs 2 floats");
    psamd::ff_minmax(ptr<float>(x), x.numel(), ptr<float>(mm), cur_stream());
  });
  m.def("ff_encode", [](Tensor x, Tensor mm, int nbytes, uint64_t seed, Tensor out) {
    chk(x, at::kFloat, "x");
    chk(mm, at::kFloat, "mm");
    chk(out, at::kByte, "out");
    check(nbytes >= 1 && nbytes <= 7, "nbytes in [1,7]");
    check(out.numel() >= x.numel() * nbytes, "out too small");
    psamd::ff_encode(ptr<float>(x), x.numel(), ptr<float>(mm), nbytes, seed, ptr<uint8_t>(out),
                     cur_stream());
  });
  m.def("ff_decode", [](Tensor code, Tensor mm, int nbytes, Tensor out) {
    chk(code, at::kByte, "code");
    chk(mm, at::kFloat, "mm");
    chk(out, at::kFloat, "out");
    check(nbytes >= 1 && nbytes <= 7, "nbytes in [1,7]");
    check(code.numel() >= out.numel() * nbytes, "code too small");
    psamd::ff_decode(ptr<uint8_t>(code), out.numel(), ptr<float>(mm), nbytes, ptr<float>(out),
                     cur_stream());
  });
  m.def("key_signature", [](Tensor keys, Tensor sig) {
    chk(keys, at::kLong, "keys");
    chk(sig, at::kLong, "sig");
    psamd::key_signature(ptr<uint64_t>(keys), keys.numel(), ptr<unsigned long long>(sig),
                         cur_stream());
  });
}
