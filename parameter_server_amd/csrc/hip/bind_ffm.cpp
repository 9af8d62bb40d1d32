// Bindings of the field-aware factorization machine (ffm.hip, ffm_csr.hip) and of its
// stored-model scoring (ffm_predict.hip).
#include "bind_common.h"
#include "ffm.h"
#include "ffm_predict.h"

using namespace psamd_bind;

namespace {

// what the two ops share: the geometry, the factor rows, the occurrences. `fields` must
// outlive the launch call (the launcher reads it on the host).
psamd::Ffm check_ffm(const Tensor& rows, const optional<Tensor>& idx, const optional<Tensor>& vals,
                     int64_t B, int S, const std::vector<int32_t>& fields, int F, int k,
                     const optional<Tensor>& local_col, const Tensor& w_local) {
  psamd::Ffm a = {};
  chk(rows, at::kBFloat16, "rows");
  chk(w_local, at::kFloat, "w_local");
  check(rows.dim() == 2, "rows [R, Dr]");
  check(S >= 1 && S <= 64, "ffm: 1..64 positions per row");
  check(k == 2 || k == 4 || k == 8, "ffm: k in {2, 4, 8}");
  a.Dr = (int)rows.size(1);
  check(rows.size(1) % 8 == 0 && rows.size(1) <= 128 && F >= 1 && (int64_t)F * k <= rows.size(1),
        "ffm: rows of F * k <= Dr <= 128 columns, Dr % 8 == 0");
  check((int64_t)fields.size() == S, "ffm: one field per position");
  for (int32_t f : fields) check(f >= 0 && f < F, "ffm: field outside [0, F)");
  check(B >= 0 && B * S < (int64_t(1) << 31), "ffm: 0 <= B * S < 2^31");
  a.B = B;
  a.S = S;
  a.F = F;
  a.k = k;
  a.fields = fields.data();
  a.local_col = optr<int32_t>(local_col, at::kInt, "local_col");
  if (a.local_col) check(local_col->numel() >= B * S, "local_col too small");
  a.vals = optr<float>(vals, at::kFloat, "vals");
  if (a.vals) check(vals->numel() >= B * S, "vals too small");
  a.rows = rows.data_ptr();
  a.rows_cap = rows.size(0);
  a.idx = optr<int64_t>(idx, at::kLong, "idx");
  a.idx_cap = a.idx ? idx->numel() : 0;
  a.w_local = ptr<float>(w_local);
  a.w_cap = w_local.numel();
  return a;
}

// the CSR ops: row_ptr [B + 1] int64, fld [nnz] int32 (device), everything per occurrence
// holds at least nnz entries
psamd::FfmCsr check_ffm_csr(const Tensor& row_ptr, const Tensor& fld, int64_t nnz,
                            const Tensor& rows, const optional<Tensor>& idx,
                            const optional<Tensor>& vals, int64_t B, int T, int F, int k,
                            const optional<Tensor>& local_col, const Tensor& w_local) {
  psamd::FfmCsr a = {};
  chk(row_ptr, at::kLong, "row_ptr");
  chk(fld, at::kInt, "fields");
  chk(rows, at::kBFloat16, "rows");
  chk(w_local, at::kFloat, "w_local");
  check(rows.dim() == 2, "rows [R, Dr]");
  check(T >= 1 && T <= 64, "ffm_csr: a tile of 1..64 rows");
  check(k == 2 || k == 4 || k == 8, "ffm_csr: k in {2, 4, 8}");
  check(rows.size(1) % 8 == 0 && rows.size(1) <= 128 && F >= 1 && (int64_t)F * k <= rows.size(1),
        "ffm_csr: rows of F * k <= Dr <= 128 columns, Dr % 8 == 0");
  check(B >= 0 && nnz >= 0 && nnz < (int64_t(1) << 31), "ffm_csr: B >= 0, 0 <= nnz < 2^31");
  check(row_ptr.numel() >= B + 1, "row_ptr too small");
  check(fld.numel() >= nnz, "fields too small");
  a.row_ptr = ptr<int64_t>(row_ptr);
  a.fld = ptr<int32_t>(fld);
  a.B = B;
  a.nnz = nnz;
  a.T = T;
  a.F = F;
  a.k = k;
  a.Dr = (int)rows.size(1);
  a.local_col = optr<int32_t>(local_col, at::kInt, "local_col");
  if (a.local_col) check(local_col->numel() >= nnz, "local_col too small");
  a.vals = optr<float>(vals, at::kFloat, "vals");
  if (a.vals) check(vals->numel() >= nnz, "vals too small");
  a.rows = rows.data_ptr();
  a.rows_cap = rows.size(0);
  a.idx = optr<int64_t>(idx, at::kLong, "idx");
  a.idx_cap = a.idx ? idx->numel() : 0;
  a.w_local = ptr<float>(w_local);
  a.w_cap = w_local.numel();
  return a;
}

}  // namespace

void psamd_bind::register_ffm(py::module_& m) {
  // CSR rows with a field per occurrence (ffm_csr.hip): rows of up to T positions on the LDS
  // tile, wider ones on the global-memory path; also writes row_of [nnz]
  m.def("ffm_csr", [](Tensor row_ptr, Tensor fld, int64_t nnz, Tensor rows, optional<Tensor> idx,
                      optional<Tensor> vals, int64_t B, int T, int F, int k,
                      optional<Tensor> local_col, Tensor w_local, Tensor labels, Tensor coef,
                      Tensor dX0, Tensor row_of, Tensor metrics, optional<Tensor> hist, int nbins) {
    psamd::FfmCsr a = check_ffm_csr(row_ptr, fld, nnz, rows, idx, vals, B, T, F, k, local_col,
                                    w_local);
    chk(labels, at::kFloat, "labels");
    chk(coef, at::kFloat, "coef");
    chk(dX0, at::kBFloat16, "dX0");
    chk(row_of, at::kInt, "row_of");
    chk(metrics, at::kDouble, "metrics");
    check(labels.numel() >= B && coef.numel() >= B, "labels/coef too small");
    check(dX0.numel() >= nnz * a.Dr, "dX0 too small");
    check(row_of.numel() >= nnz, "row_of too small");
    check(metrics.numel() >= 3, "metrics[3]");
    a.hist = optr<uint32_t>(hist, at::kInt, "hist");
    if (a.hist) check(nbins > 0 && hist->numel() >= 2 * nbins, "hist too small");
    a.labels = ptr<float>(labels);
    a.coef = ptr<float>(coef);
    a.dX0 = dX0.data_ptr();
    a.row_of = ptr<int32_t>(row_of);
    a.metrics = ptr<double>(metrics);
    a.nbins = nbins;
    a.acc_stripes = acc_stripes_of(metrics);
    psamd::ffm_csr(a, cur_stream());
  });
  m.def("ffm_csr_margins", [](Tensor row_ptr, Tensor fld, int64_t nnz, Tensor rows,
                              optional<Tensor> idx, optional<Tensor> vals, int64_t B, int T, int F,
                              int k, optional<Tensor> local_col, Tensor w_local, Tensor margins) {
    psamd::FfmCsr a = check_ffm_csr(row_ptr, fld, nnz, rows, idx, vals, B, T, F, k, local_col,
                                    w_local);
    chk(margins, at::kFloat, "margins");
    check(margins.numel() >= B, "margins too small");
    a.margins = ptr<float>(margins);
    psamd::ffm_csr_margins(a, cur_stream());
  });
  // rows [R, Dr] bf16 read through local_col (None: column = position) and idx (None: the
  // column is the row); fields [S] ints in [0, F), one map for all rows
  m.def("ffm_fwd_bwd", [](Tensor rows, optional<Tensor> idx, optional<Tensor> vals, int64_t B,
                          int S, std::vector<int32_t> fields, int F, int k,
                          optional<Tensor> local_col, Tensor w_local, Tensor labels, Tensor coef,
                          Tensor dX0, Tensor metrics, optional<Tensor> hist, int nbins) {
    psamd::Ffm a = check_ffm(rows, idx, vals, B, S, fields, F, k, local_col, w_local);
    chk(labels, at::kFloat, "labels");
    chk(coef, at::kFloat, "coef");
    chk(dX0, at::kBFloat16, "dX0");
    chk(metrics, at::kDouble, "metrics");
    check(labels.numel() >= B && coef.numel() >= B, "labels/coef too small");
    check(dX0.numel() >= B * S * a.Dr, "dX0 too small");
    check(metrics.numel() >= 3, "metrics[3]");
    a.hist = optr<uint32_t>(hist, at::kInt, "hist");
    if (a.hist) check(nbins > 0 && hist->numel() >= 2 * nbins, "hist too small");
    a.labels = ptr<float>(labels);
    a.coef = ptr<float>(coef);
    a.dX0 = dX0.data_ptr();
    a.metrics = ptr<double>(metrics);
    a.nbins = nbins;
    a.acc_stripes = acc_stripes_of(metrics);
    psamd::ffm_fwd_bwd(a, cur_stream());
  });
  // the forward-only form: margins [B] and nothing else
  m.def("ffm_margins", [](Tensor rows, optional<Tensor> idx, optional<Tensor> vals, int64_t B,
                          int S, std::vector<int32_t> fields, int F, int k,
                          optional<Tensor> local_col, Tensor w_local, Tensor margins) {
    psamd::Ffm a = check_ffm(rows, idx, vals, B, S, fields, F, k, local_col, w_local);
    chk(margins, at::kFloat, "margins");
    check(margins.numel() >= B, "margins too small");
    a.margins = ptr<float>(margins);
    psamd::ffm_margins(a, cur_stream());
  });
  // Scoring a stored FFM from raw keys (ffm_predict.hip), the arguments of fm_predict_rows
  // plus F, k and the fields: with row_ptr, fields [nnz] int32 (one per occurrence); with a
  // fixed width, field_of [width] int32 (position -> field; None: the position is the field).
  // metrics / hist need labels.
  m.def("ffm_predict_rows", [](Tensor slots, uint64_t home_base, uint64_t home_m, Tensor rows,
                               Tensor keys, int bits, int F, int k, optional<Tensor> row_ptr,
                               int width, optional<Tensor> fields, optional<Tensor> field_of,
                               optional<Tensor> vals, optional<Tensor> labels, int64_t B,
                               int loss_type, optional<Tensor> margin, optional<Tensor> metrics,
                               optional<Tensor> hist, int nbins) {
    const std::string op = "ffm_predict_rows: ";
    const psamd::TableRef t = table_ref(slots, home_base, home_m);
    chk(rows, at::kBFloat16, "rows");
    chk(keys, at::kLong, "keys");
    check(rows.dim() == 2 && rows.size(0) == t.cap, op + "rows must be [table capacity, Dr]");
    const int64_t nnz = keys.numel();
    check(B >= 0, op + "B >= 0");
    const int64_t* rp = optr<int64_t>(row_ptr, at::kLong, "row_ptr");
    if (rp) check(row_ptr->numel() >= B + 1, "row_ptr too small");
    else check(width > 0 && B <= nnz / width, "fixed width layout too small");
    const int32_t* fl = optr<int32_t>(fields, at::kInt, "fields");
    if (fl) check(fields->numel() >= nnz, "fields too small");
    const int32_t* fo = optr<int32_t>(field_of, at::kInt, "field_of");
    const float* v = optr<float>(vals, at::kFloat, "vals");
    if (v) check(vals->numel() >= nnz, "vals too small");
    const float* lb = optr<float>(labels, at::kFloat, "labels");
    if (lb) check(labels->numel() >= B, "labels too small");
    float* mg = optr<float>(margin, at::kFloat, "margin");
    if (mg) check(margin->numel() >= B, "margin too small");
    const psamd::StripedAcc acc = striped_acc(metrics, "metrics");
    if (acc.ptr) check(lb && metrics->numel() >= 3, "metrics needs labels and >= 3 slots");
    auto* hp = optr<unsigned long long>(hist, at::kLong, "hist");
    if (hp) check(lb && nbins > 0 && nbins <= 8192 && hist->numel() >= 2 * nbins &&
                      hist->numel() % (2 * nbins) == 0,
                  "hist needs labels and int64 [stripes x 2 x nbins], nbins <= 8192");
    check(loss_type >= 1 && loss_type <= 4, "loss type in [1, 4]");
    psamd::ffm_predict_rows(t, make_keymix(bits), rows.data_ptr(), (int)rows.size(1), F, k,
                            ptr<uint64_t>(keys), nnz, rp, width, fl, fo,
                            fo ? field_of->numel() : 0, v, lb, B, loss_type, mg, acc, hp, nbins,
                            hp ? (int)(hist->numel() / (2 * nbins)) : 1, cur_stream());
  }, py::arg("slots"), py::arg("home_base"), py::arg("home_m"), py::arg("rows"), py::arg("keys"),
     py::arg("bits"), py::arg("F"), py::arg("k"), py::arg("row_ptr"), py::arg("width"),
     py::arg("fields"), py::arg("field_of"), py::arg("vals"), py::arg("labels"), py::arg("B"),
     py::arg("loss_type"), py::arg("margin"), py::arg("metrics"), py::arg("hist"),
     py::arg("nbins"));
}
