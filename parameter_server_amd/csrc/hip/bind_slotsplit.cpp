// Bindings of the split by feature group (slotsplit.hip).
#include "bind_common.h"
#include "slotsplit.h"

using namespace psamd_bind;

void psamd_bind::register_slotsplit(py::module_& m) {
  m.def("slotsplit_tile", [] { return psamd::slotsplit_tile(); });
  m.def("slotsplit_max_ids", [] { return psamd::slotsplit_max_ids(); });
  m.def("slotsplit_default_cell_cap", [] { return psamd::slotsplit_default_cell_cap(); });
  m.def("slotsplit_hdr_words", [] { return psamd::slotsplit_hdr_words(); });
  m.def("slotsplit_work_words", [](int64_t nnz, int64_t cells) {
    check(nnz >= 0 && cells >= 0, "slotsplit_work_words: negative size");
    return psamd::slotsplit_work_words(nnz, cells);
  });
  // row_ptr [R + 1], keys / vals (None: binary) / slots [nnz] -> keys_out / vals_out [nnz]
  // slot-major; hdr = {S, flags, cells, total, ..., ids[4096], totals[4096]}. cells: the
  // size of the cell arrays in work; cell_cap <= cells.
  m.def("slotsplit", [](Tensor row_ptr, Tensor keys, optional<Tensor> vals, Tensor slots,
                        int64_t cell_cap, int64_t cells, Tensor keys_out,
                        optional<Tensor> vals_out, Tensor hdr, Tensor work) {
    chk(row_ptr, at::kLong, "row_ptr");
    chk(keys, at::kLong, "keys");
    chk(slots, at::kInt, "slots");
    chk(keys_out, at::kLong, "keys_out");
    chk(hdr, at::kInt, "hdr");
    chk(work, at::kInt, "work");
    const int64_t R = row_ptr.numel() - 1, n = keys.numel();
    check(R >= 1 && n >= 1, "slotsplit: needs a row and an entry");
    check(slots.numel() == n && keys_out.numel() >= n, "slotsplit: slots / keys_out [nnz]");
    const float* vp = optr<float>(vals, at::kFloat, "vals");
    float* vo = optr<float>(vals_out, at::kFloat, "vals_out");
    check((vp == nullptr) == (vo == nullptr), "slotsplit: vals and vals_out go together");
    if (vp) check(vals->numel() == n && vals_out->numel() >= n, "slotsplit: vals / vals_out [nnz]");
    check(hdr.numel() >= psamd::slotsplit_hdr_words(), "slotsplit: header too small");
    check(cells >= 1 && cells <= ((int64_t)1 << 30) && cell_cap >= 0 && cell_cap <= cells,
          "slotsplit: 0 <= cell_cap <= cells <= 2^30");
    check(work.numel() >= psamd::slotsplit_work_words(n, cells), "slotsplit: work buffer too small");
    psamd::slotsplit(ptr<int64_t>(row_ptr), R, ptr<uint64_t>(keys), vp, ptr<int32_t>(slots), n,
                     cell_cap, cells, ptr<uint64_t>(keys_out), vo, ptr<int32_t>(hdr),
                     ptr<int32_t>(work), cur_stream());
  });
  m.def("slotsplit_offsets", [](Tensor work, int64_t nnz, int64_t cells, int64_t R, int64_t S,
                                Tensor off) {
    chk(work, at::kInt, "work");
    chk(off, at::kLong, "off");
    check(nnz >= 1 && R >= 1 && cells >= 1 && cells <= ((int64_t)1 << 30),
          "slotsplit_offsets: sizes");
    check(work.numel() >= psamd::slotsplit_work_words(nnz, cells),
          "slotsplit_offsets: work buffer too small");
    check(S >= 1 && S <= psamd::slotsplit_max_ids() && S * R <= cells,
          "slotsplit_offsets: S groups of R rows outside the work space");
    check(off.numel() >= S * (R + 1), "slotsplit_offsets: off [S, R + 1]");
    psamd::slotsplit_offsets(ptr<int32_t>(work), nnz, cells, R, S, ptr<int64_t>(off), cur_stream());
  });
}
