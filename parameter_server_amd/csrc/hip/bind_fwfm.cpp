// Bindings of the field-weighted factorization machine (fwfm.hip, fwfm_csr.hip) and of its
// stored-model scoring (fwfm_predict.hip).
#include "bind_common.h"
#include "fwfm.h"
#include "fwfm_predict.h"

using namespace psamd_bind;

namespace {

int padded_fields(int F) { return (F + 15) / 16 * 16; }

// what the two row ops share: the geometry, the factor rows, the occurrences, R. `fields`
// must outlive the launch call (the launcher reads it on the host).
psamd::Fwfm check_fwfm(const Tensor& rows, const optional<Tensor>& idx,
                       const optional<Tensor>& vals, int64_t B, int S,
                       const std::vector<int32_t>& fields, int F, const Tensor& R,
                       const optional<Tensor>& local_col, const Tensor& w_local) {
  psamd::Fwfm a = {};
  chk(rows, at::kBFloat16, "rows");
  chk(w_local, at::kFloat, "w_local");
  chk(R, at::kFloat, "R");
  check(rows.dim() == 2, "rows [R, D]");
  check(S >= 1 && S <= 64, "fwfm: 1..64 positions per row");
  check(F >= 1 && F <= 64, "fwfm: 1..64 fields");
  check(rows.size(1) == 8 || rows.size(1) == 16 || rows.size(1) == 32,
        "fwfm: rows of D in {8, 16, 32} columns");
  check(R.numel() == (int64_t)F * F, "fwfm: R [F, F]");
  check((int64_t)fields.size() == S, "fwfm: one field per position");
  for (int32_t f : fields) check(f >= 0 && f < F, "fwfm: field outside [0, F)");
  check(B >= 0 && B * S < (int64_t(1) << 31), "fwfm: 0 <= B * S < 2^31");
  a.B = B;
  a.S = S;
  a.F = F;
  a.Dr = (int)rows.size(1);
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
  a.R = ptr<float>(R);
  return a;
}

// the CSR ops: row_ptr [B + 1] int64, fld [nnz] int32 (device), everything per occurrence
// holds at least nnz entries
psamd::FwfmCsr check_fwfm_csr(const Tensor& row_ptr, const Tensor& fld, int64_t nnz,
                              const Tensor& rows, const optional<Tensor>& idx,
                              const optional<Tensor>& vals, int64_t B, int F, const Tensor& R,
                              const optional<Tensor>& local_col, const Tensor& w_local) {
  psamd::FwfmCsr a = {};
  chk(row_ptr, at::kLong, "row_ptr");
  chk(fld, at::kInt, "fields");
  chk(rows, at::kBFloat16, "rows");
  chk(w_local, at::kFloat, "w_local");
  chk(R, at::kFloat, "R");
  check(rows.dim() == 2, "rows [R, D]");
  check(F >= 1 && F <= 64, "fwfm_csr: 1..64 fields");
  check(rows.size(1) == 8 || rows.size(1) == 16 || rows.size(1) == 32,
        "fwfm_csr: rows of D in {8, 16, 32} columns");
  check(R.numel() == (int64_t)F * F, "fwfm_csr: R [F, F]");
  check(B >= 0 && nnz >= 0 && nnz < (int64_t(1) << 31), "fwfm_csr: B >= 0, 0 <= nnz < 2^31");
  check(row_ptr.numel() >= B + 1, "row_ptr too small");
  check(fld.numel() >= nnz, "fields too small");
  a.row_ptr = ptr<int64_t>(row_ptr);
  a.fld = ptr<int32_t>(fld);
  a.B = B;
  a.nnz = nnz;
  a.F = F;
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
  a.R = ptr<float>(R);
  return a;
}

// dR_part [parts, Fp * Fp] f32: the number of partials is the tensor's first dimension
int check_parts(const Tensor& dR_part, int F) {
  chk(dR_part, at::kFloat, "dR_part");
  const int64_t fp2 = (int64_t)padded_fields(F) * padded_fields(F);
  check(dR_part.dim() == 2 && dR_part.size(1) == fp2 && dR_part.size(0) >= 1 &&
            dR_part.size(0) <= 4096,
        "fwfm: dR_part [1..4096, Fp * Fp], Fp = F rounded up to 16");
  return (int)dR_part.size(0);
}

}  // namespace

void psamd_bind::register_fwfm(py::module_& m) {
  // rows [R, D] bf16 read through local_col (None: column = position) and idx (None: the
  // column is the row); fields [S] ints in [0, F), one map for all rows; R [F, F] f32, read
  // as symmetric from its upper triangle. One block per row of dR_part, each writes its
  // partial of dR (fwfm_dr_reduce sums them).
  m.def("fwfm_fwd_bwd", [](Tensor rows, optional<Tensor> idx, optional<Tensor> vals, int64_t B,
                           int S, std::vector<int32_t> fields, int F, Tensor R,
                           optional<Tensor> local_col, Tensor w_local, Tensor labels, Tensor coef,
                           Tensor dX0, Tensor dR_part, Tensor metrics, optional<Tensor> hist,
                           int nbins) {
    psamd::Fwfm a = check_fwfm(rows, idx, vals, B, S, fields, F, R, local_col, w_local);
    chk(labels, at::kFloat, "labels");
    chk(coef, at::kFloat, "coef");
    chk(dX0, at::kBFloat16, "dX0");
    chk(metrics, at::kDouble, "metrics");
    check(labels.numel() >= B && coef.numel() >= B, "labels/coef too small");
    check(dX0.numel() >= B * S * a.Dr, "dX0 too small");
    check(metrics.numel() >= 3, "metrics[3]");
    a.parts = check_parts(dR_part, F);
    a.dR_part = ptr<float>(dR_part);
    a.hist = optr<uint32_t>(hist, at::kInt, "hist");
    if (a.hist) check(nbins > 0 && hist->numel() >= 2 * nbins, "hist too small");
    a.labels = ptr<float>(labels);
    a.coef = ptr<float>(coef);
    a.dX0 = dX0.data_ptr();
    a.metrics = ptr<double>(metrics);
    a.nbins = nbins;
    a.acc_stripes = acc_stripes_of(metrics);
    psamd::fwfm_fwd_bwd(a, cur_stream());
  });
  // the forward-only form: margins [B] and nothing else
  m.def("fwfm_margins", [](Tensor rows, optional<Tensor> idx, optional<Tensor> vals, int64_t B,
                           int S, std::vector<int32_t> fields, int F, Tensor R,
                           optional<Tensor> local_col, Tensor w_local, Tensor margins) {
    psamd::Fwfm a = check_fwfm(rows, idx, vals, B, S, fields, F, R, local_col, w_local);
    chk(margins, at::kFloat, "margins");
    check(margins.numel() >= B, "margins too small");
    a.margins = ptr<float>(margins);
    psamd::fwfm_margins(a, cur_stream());
  });
  // CSR rows of any width with a field per occurrence (fwfm_csr.hip): row_ptr [B + 1] int64,
  // fld [nnz] int32; also writes row_of [nnz]. One block per row of dR_part, as fwfm_fwd_bwd.
  m.def("fwfm_csr", [](Tensor row_ptr, Tensor fld, int64_t nnz, Tensor rows, optional<Tensor> idx,
                       optional<Tensor> vals, int64_t B, int F, Tensor R,
                       optional<Tensor> local_col, Tensor w_local, Tensor labels, Tensor coef,
                       Tensor dX0, Tensor row_of, Tensor dR_part, Tensor metrics,
                       optional<Tensor> hist, int nbins) {
    psamd::FwfmCsr a = check_fwfm_csr(row_ptr, fld, nnz, rows, idx, vals, B, F, R, local_col,
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
    a.parts = check_parts(dR_part, F);
    a.dR_part = ptr<float>(dR_part);
    a.hist = optr<uint32_t>(hist, at::kInt, "hist");
    if (a.hist) check(nbins > 0 && hist->numel() >= 2 * nbins, "hist too small");
    a.labels = ptr<float>(labels);
    a.coef = ptr<float>(coef);
    a.dX0 = dX0.data_ptr();
    a.row_of = ptr<int32_t>(row_of);
    a.metrics = ptr<double>(metrics);
    a.nbins = nbins;
    a.acc_stripes = acc_stripes_of(metrics);
    psamd::fwfm_csr_fwd_bwd(a, cur_stream());
  });
  m.def("fwfm_csr_margins", [](Tensor row_ptr, Tensor fld, int64_t nnz, Tensor rows,
                               optional<Tensor> idx, optional<Tensor> vals, int64_t B, int F,
                               Tensor R, optional<Tensor> local_col, Tensor w_local,
                               Tensor margins) {
    psamd::FwfmCsr a = check_fwfm_csr(row_ptr, fld, nnz, rows, idx, vals, B, F, R, local_col,
                                      w_local);
    chk(margins, at::kFloat, "margins");
    check(margins.numel() >= B, "margins too small");
    a.margins = ptr<float>(margins);
    psamd::fwfm_csr_margins(a, cur_stream());
  });
  // sum: dR [F, F] = the partials in a fixed order, mirrored. update: AdaGrad on R and acc
  // [F, F] with g = dR + lambda_r R. Both in one launch on one rank; sum, an all-reduce of
  // dR, then update on several.
  m.def("fwfm_dr_reduce", [](optional<Tensor> dR_part, Tensor dR, int F, bool sum, bool update,
                             optional<Tensor> R, optional<Tensor> acc, double lr,
                             double lambda_r) {
    psamd::FwfmReduce a = {};
    check(F >= 1 && F <= 64, "fwfm_dr_reduce: 1..64 fields");
    check(sum || update, "fwfm_dr_reduce: sum, update or both");
    chk(dR, at::kFloat, "dR");
    check(dR.numel() == (int64_t)F * F, "fwfm_dr_reduce: dR [F, F]");
    a.F = F;
    a.dR = ptr<float>(dR);
    a.sum = sum;
    a.update = update;
    if (sum) {
      check(dR_part.has_value() && dR_part->defined(), "fwfm_dr_reduce: sum needs dR_part");
      a.parts = check_parts(*dR_part, F);
      a.dR_part = ptr<float>(*dR_part);
    }
    if (update) {
      a.R = optr<float>(R, at::kFloat, "R");
      a.acc = optr<float>(acc, at::kFloat, "acc");
      check(a.R && a.acc && R->numel() == (int64_t)F * F && acc->numel() == (int64_t)F * F,
            "fwfm_dr_reduce: the update needs R and acc [F, F]");
      check(lr > 0, "fwfm_dr_reduce: lr > 0");
      a.lr = (float)lr;
      a.lambda_r = (float)lambda_r;
    }
    psamd::fwfm_dr_reduce(a, cur_stream());
  }, py::arg("dR_part"), py::arg("dR"), py::arg("F"), py::arg("sum"), py::arg("update"),
     py::arg("R") = py::none(), py::arg("acc") = py::none(), py::arg("lr") = 0.0,
     py::arg("lambda_r") = 0.0);
  // Scoring a stored FwFM from raw keys (fwfm_predict.hip), the arguments of ffm_predict_rows
  // with R [F, F] f32 in the place of k: with row_ptr, fields [nnz] int32 (one per
  // occurrence); with a fixed width, field_of [width] int32 (position -> field; None: the
  // position is the field). metrics / hist need labels.
  m.def("fwfm_predict_rows", [](Tensor slots, uint64_t home_base, uint64_t home_m, Tensor rows,
                                Tensor keys, int bits, int F, Tensor R, optional<Tensor> row_ptr,
                                int width, optional<Tensor> fields, optional<Tensor> field_of,
                                optional<Tensor> vals, optional<Tensor> labels, int64_t B,
                                int loss_type, optional<Tensor> margin, optional<Tensor> metrics,
                                optional<Tensor> hist, int nbins) {
    const std::string op = "fwfm_predict_rows: ";
    const psamd::TableRef t = table_ref(slots, home_base, home_m);
    chk(rows, at::kBFloat16, "rows");
    chk(keys, at::kLong, "keys");
    chk(R, at::kFloat, "R");
    check(rows.dim() == 2 && rows.size(0) == t.cap, op + "rows must be [table capacity, D]");
    check(F >= 1 && F <= 64 && R.numel() == (int64_t)F * F, op + "R [F, F], 1..64 fields");
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
    psamd::fwfm_predict_rows(t, make_keymix(bits), rows.data_ptr(), (int)rows.size(1), F,
                             ptr<float>(R), ptr<uint64_t>(keys), nnz, rp, width, fl, fo,
                             fo ? field_of->numel() : 0, v, lb, B, loss_type, mg, acc, hp, nbins,
                             hp ? (int)(hist->numel() / (2 * nbins)) : 1, cur_stream());
  }, py::arg("slots"), py::arg("home_base"), py::arg("home_m"), py::arg("rows"), py::arg("keys"),
     py::arg("bits"), py::arg("F"), py::arg("R"), py::arg("row_ptr"), py::arg("width"),
     py::arg("fields"), py::arg("field_of"), py::arg("vals"), py::arg("labels"), py::arg("B"),
     py::arg("loss_type"), py::arg("margin"), py::arg("metrics"), py::arg("hist"),
     py::arg("nbins"));
}
