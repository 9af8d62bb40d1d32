// Bindings of the linear model (linear.hip), stored-model scoring (predict.hip), the
// factorization machine (fm.hip) and the synthetic Criteo generator.
#include <memory>

#include "bind_common.h"
#include "fm.h"
#include "linear.h"
#include "predict.h"

using namespace psamd_bind;

namespace {

// the generator's buffers, checked alike by the eager op and the list op
void check_criteo_gen(const Tensor& keys, const Tensor& labels, int64_t B, double alpha) {
  chk(keys, at::kLong, "keys");
  chk(labels, at::kFloat, "labels");
  check(keys.numel() >= B * 39 && labels.numel() >= B, "criteo_gen buffers too small");
  check(alpha > 1.0, "power-law alpha must be > 1");
}

// Synthetic minibatch generator with a row cursor kept in the launcher: run k uses rows
// [row0 + k * row_step, + B) (a prepared-minibatch buffer is refilled every row_step / B
// minibatches), so a launch list regenerates fresh data on every run with the row offset
// as a plain launch argument (no device counter, no extra launch).
Launch make_criteo_gen(uint64_t seed, int64_t row0, int64_t row_step, int64_t B,
                       uint64_t num_features, double alpha, Tensor keys, Tensor labels) {
  check_criteo_gen(keys, labels, B, alpha);
  check(num_features > 0 && B > 0, "num_features > 0, B > 0");
  auto cursor = std::make_shared<int64_t>(row0);
  return [=, keep = std::vector<Tensor>{keys, labels}](hipStream_t st) {
    psamd::criteo_gen(seed, *cursor, nullptr, 1, B, num_features, (float)alpha,
                      ptr<uint64_t>(keys), ptr<float>(labels), nullptr, st);
    *cursor += row_step;
  };
}

// what the two FM forward / backward ops share (X0 expanded, or rows gathered): the
// dtype checks, then the sizes and the optional vals / hist
struct FmArgs {
  const float* v;
  uint32_t* h;
};
void check_fm(const Tensor& dX0, const Tensor& local_col, const Tensor& w_local,
              const Tensor& labels, const Tensor& coef, const Tensor& metrics) {
  chk(dX0, at::kBFloat16, "dX0");
  chk(local_col, at::kInt, "local_col");
  chk(w_local, at::kFloat, "w_local");
  chk(labels, at::kFloat, "labels");
  chk(coef, at::kFloat, "coef");
  chk(metrics, at::kDouble, "metrics");
}
FmArgs check_fm_sizes(const Tensor& local_col, const Tensor& labels, const Tensor& coef,
                      const Tensor& metrics, const optional<Tensor>& vals,
                      const optional<Tensor>& hist, int64_t B, int S, int nbins) {
  check(local_col.numel() >= B * S && labels.numel() >= B && coef.numel() >= B, "too small");
  check(metrics.numel() >= 3, "metrics[3]");
  FmArgs a;
  a.v = optr<float>(vals, at::kFloat, "vals");
  if (a.v) check(vals->numel() >= B * S, "vals too small");
  a.h = optr<uint32_t>(hist, at::kInt, "hist");
  if (a.h) check(hist->numel() >= 2 * nbins, "hist too small");
  return a;
}

}  // namespace

void psamd_bind::register_linear(py::module_& m) {
  // ---------------- linear model ----------------
  m.def("linear_fwd", [](optional<Tensor> row_ptr, int64_t B, int width, Tensor local_col,
                         optional<Tensor> vals, Tensor w_local, Tensor labels, int loss_type,
                         optional<Tensor> xw, Tensor coef, optional<Tensor> coef2,
                         optional<Tensor> metrics, optional<Tensor> hist, int nbins) {
    chk(local_col, at::kInt, "local_col");
    chk(w_local, at::kFloat, "w_local");
    chk(labels, at::kFloat, "labels");
    chk(coef, at::kFloat, "coef");
    check(labels.numel() >= B && coef.numel() >= B, "labels/coef too small");
    const int64_t* rp = optr<int64_t>(row_ptr, at::kLong, "row_ptr");
    if (rp) check(row_ptr->numel() >= B + 1, "row_ptr too small");
    else check(width > 0 && local_col.numel() >= B * width, "fixed width layout too small");
    const float* v = optr<float>(vals, at::kFloat, "vals");
    if (v) check(vals->numel() >= local_col.numel(), "vals too small");
    uint32_t* hp = optr<uint32_t>(hist, at::kInt, "hist");
    if (hp) check(nbins > 0 && nbins <= 8192 && hist->numel() >= 2 * nbins, "hist size");
    float* xp = optr<float>(xw, at::kFloat, "xw");
    if (xp) check(xw->numel() >= B, "xw too small");
    float* c2 = optr<float>(coef2, at::kFloat, "coef2");
    if (c2) check(coef2->numel() >= B, "coef2 too small");
    double* mp = optr<double>(metrics, at::kDouble, "metrics");
    if (mp) check(metrics->numel() >= 5, "metrics needs >= 5 slots");
    psamd::linear_fwd(rp, B, width, ptr<int32_t>(local_col), v, ptr<float>(w_local),
                      w_local.numel(), ptr<float>(labels), loss_type, xp, ptr<float>(coef), c2, mp,
                      hp, nbins, acc_stripes_of(metrics),
                      hp ? (int)std::max<int64_t>(1, hist->numel() / (2 * nbins)) : 1,
                      cur_stream());
  });
  // Score a minibatch of raw keys against a slot table (predict.hip): margin[B], the
  // striped [loss, correct, count] sums and the u64 striped AUC histogram, each optional.
  // lanes: lanes per row, 0 = from nnz / B (predict.hip predict_lanes), else 8 or 64.
  m.def("predict_rows", [](Tensor slots, uint64_t home_base, uint64_t home_m, Tensor keys,
                           int bits, optional<Tensor> row_ptr, int width, optional<Tensor> vals,
                           optional<Tensor> labels, int64_t B, int loss_type,
                           optional<Tensor> margin, optional<Tensor> metrics,
                           optional<Tensor> hist, int nbins, int lanes) {
    const psamd::TableRef t = table_ref(slots, home_base, home_m);
    chk(keys, at::kLong, "keys");
    const int64_t nnz = keys.numel();
    check(B >= 0, "predict_rows: B >= 0");
    const int64_t* rp = optr<int64_t>(row_ptr, at::kLong, "row_ptr");
    if (rp) check(row_ptr->numel() >= B + 1, "row_ptr too small");
    else check(width > 0 && B <= nnz / width, "fixed width layout too small");
    const float* v = optr<float>(vals, at::kFloat, "vals");
    if (v) check(vals->numel() >= nnz, "vals too small");
    const float* lb = optr<float>(labels, at::kFloat, "labels");
    if (lb) check(labels->numel() >= B, "labels too small");
    float* mg = optr<float>(margin, at::kFloat, "margin");
    if (mg) check(margin->numel() >= B, "margin too small");
    const psamd::StripedAcc acc = striped_acc(metrics, "metrics");
    if (acc.ptr) check(lb && metrics->numel() >= 3, "metrics needs labels and >= 3 slots");
    unsigned long long* hp = optr<unsigned long long>(hist, at::kLong, "hist");
    if (hp) check(lb && nbins > 0 && nbins <= 8192 && hist->numel() >= 2 * nbins &&
                      hist->numel() % (2 * nbins) == 0,
                  "hist needs labels and int64 [stripes x 2 x nbins], nbins <= 8192");
    check(lanes == 0 || lanes == 8 || lanes == 64, "lanes per row: 0 (auto), 8 or 64");
    check(loss_type >= 1 && loss_type <= 4, "loss type in [1, 4]");
    psamd::predict_rows(t, make_keymix(bits), ptr<uint64_t>(keys), nnz, rp, width, v, lb, B,
                        loss_type, mg, acc, hp, nbins,
                        hp ? (int)(hist->numel() / (2 * nbins)) : 1, lanes, cur_stream());
  }, py::arg("slots"), py::arg("home_base"), py::arg("home_m"), py::arg("keys"), py::arg("bits"),
     py::arg("row_ptr"), py::arg("width"), py::arg("vals"), py::arg("labels"), py::arg("B"),
     py::arg("loss_type"), py::arg("margin"), py::arg("metrics"), py::arg("hist"),
     py::arg("nbins"), py::arg("lanes") = 0);
  m.def("linear_bwd", [](Tensor pos_s, Tensor segid, int64_t n, optional<Tensor> rows, int width,
                         optional<Tensor> vals, Tensor coef, optional<Tensor> coef2, Tensor grad,
                         optional<Tensor> hess) {
    chk(pos_s, at::kInt, "pos_s");
    chk(segid, at::kInt, "segid");
    chk(coef, at::kFloat, "coef");
    chk(grad, at::kFloat, "grad");
    check(pos_s.numel() >= n && segid.numel() >= n, "bwd inputs too small");
    const int32_t* r = optr<int32_t>(rows, at::kInt, "rows");
    if (r) check(rows->numel() >= n, "rows too small");
    else check(width > 0, "need rows or a fixed width");
    float* h = optr<float>(hess, at::kFloat, "hess");
    const float* c2 = optr<float>(coef2, at::kFloat, "coef2");
    check(!h || c2, "hess requires coef2");
    if (h) check(hess->numel() >= grad.numel(), "hess smaller than grad");
    psamd::linear_bwd(ptr<int32_t>(pos_s), ptr<int32_t>(segid), n, r, width,
                      optr<float>(vals, at::kFloat, "vals"), ptr<float>(coef), coef.numel(), c2,
                      ptr<float>(grad), h, grad.numel(), cur_stream());
  });
  m.def("auc_from_hist", [](Tensor hist, int nbins, Tensor metrics,
                            optional<Tensor> step_counter) {
    chk(hist, at::kInt, "hist");
    chk(metrics, at::kDouble, "metrics");
    check(hist.numel() >= 2 * nbins && metrics.numel() >= 5, "auc sizes");
    check(nbins == 2048, "auc_from_hist: 2048 bins (256 threads x 8)");
    const int stripes = (int)std::max<int64_t>(1, hist.numel() / (2 * nbins));
    check(stripes <= 8, "auc_from_hist: at most 8 histogram stripes");
    psamd::auc_from_hist({ptr<uint32_t>(hist), nbins, stripes, ptr<double>(metrics),
                          optr<int64_t>(step_counter, at::kLong, "step_counter")},
                         cur_stream());
  }, py::arg("hist"), py::arg("nbins"), py::arg("metrics"),
     py::arg("step_counter") = py::none());
  m.def("csr_rows", [](Tensor row_ptr, Tensor rows) {
    chk(row_ptr, at::kLong, "row_ptr");
    chk(rows, at::kInt, "rows");
    psamd::csr_rows(ptr<int64_t>(row_ptr), row_ptr.numel() - 1, ptr<int32_t>(rows),
                    cur_stream());
  });
  m.def("criteo_set_tables", [](std::vector<uint32_t> cards, std::vector<float> gauss) {
    check(cards.size() == 26, "need 26 cardinalities");
    check(gauss.size() == 256, "need 256 Gaussian quantiles");
    psamd::criteo_set_tables(cards.data(), gauss.data());
  });
  m.def("add_i64", [](Tensor p, int64_t v) {
    chk(p, at::kLong, "p");
    psamd::add_i64(ptr<int64_t>(p), v, cur_stream());
  });
  // (the Python API is fixed: the eager op takes a device cursor, the list op keeps its
  // own row cursor and step)
  m.def("criteo_gen", [](uint64_t seed, int64_t row0, int64_t B, uint64_t num_features,
                         double alpha, Tensor keys, Tensor labels, optional<Tensor> row0_dev,
                         int64_t row_scale, optional<Tensor> row0_out) {
    // row0_out: the kernel writes row0_dev + 1 there (the cursor of the next launch, which
    // reads row0_out and writes row0_dev: a captured graph pair alternating the two
    // words generates fresh rows on every replay, no separate add)
    int64_t* op = optr<int64_t>(row0_out, at::kLong, "row0_out");
    if (op) check(row0_dev.has_value() && row0_dev->defined() && row0_out->numel() >= 1 &&
                      row0_dev->numel() >= 1 && op != row0_dev->data_ptr<int64_t>(),
                  "row0_out: a word of its own next to row0_dev");
    check_criteo_gen(keys, labels, B, alpha);
    check(num_features > 0, "num_features > 0");
    psamd::criteo_gen(seed, row0, optr<int64_t>(row0_dev, at::kLong, "row0_dev"), row_scale, B,
                      num_features, (float)alpha, ptr<uint64_t>(keys), ptr<float>(labels),
                      op, cur_stream());
  }, py::arg("seed"), py::arg("row0"), py::arg("B"), py::arg("num_features"), py::arg("alpha"),
     py::arg("keys"), py::arg("labels"), py::arg("row0_dev") = py::none(),
     py::arg("row_scale") = 1, py::arg("row0_out") = py::none());
  launch_list_class(m).def("add_criteo_gen", [](LaunchList& l, uint64_t seed, int64_t row0,
                                                int64_t row_step, int64_t B,
                                                uint64_t num_features, double alpha, Tensor keys,
                                                Tensor labels) {
    l.push(make_criteo_gen(seed, row0, row_step, B, num_features, alpha, keys, labels),
           "criteo_gen");
  });

  // ---------------- factorization machine (fm.hip) ----------------
  m.def("fm_fwd_bwd", [](Tensor X0, optional<Tensor> vals, int64_t B, int S, Tensor local_col,
                         Tensor w_local, Tensor labels, Tensor coef, Tensor dX0, Tensor metrics,
                         optional<Tensor> hist, int nbins) {
    chk(X0, at::kBFloat16, "X0");
    check_fm(dX0, local_col, w_local, labels, coef, metrics);
    check(X0.dim() == 2 && X0.size(1) <= 128 && X0.size(1) > 0, "X0 must be [B*S, D<=128]");
    check(S > 0 && S <= 64, "1..64 keys per example");
    const int D = (int)X0.size(1);
    check(X0.size(0) >= B * S && dX0.numel() >= B * S * D, "X0/dX0 too small");
    const FmArgs a = check_fm_sizes(local_col, labels, coef, metrics, vals, hist, B, S, nbins);
    psamd::fm_fwd_bwd(X0.data_ptr(), nullptr, nullptr, 0, 0, a.v, B, S, D, ptr<int32_t>(local_col),
                      ptr<float>(w_local), w_local.numel(), ptr<float>(labels), ptr<float>(coef),
                      dX0.data_ptr(), ptr<double>(metrics), a.h, nbins, acc_stripes_of(metrics),
                      cur_stream());
  });
  m.def("fm_fwd_bwd_gather", [](Tensor rows, optional<Tensor> idx, optional<Tensor> vals, int64_t B,
                                int S, Tensor local_col, Tensor w_local, Tensor labels, Tensor coef,
                                Tensor dX0, Tensor metrics, optional<Tensor> hist, int nbins) {
    // rows [R, D] bf16 read through local_col (and idx) -- no expanded X0
    chk(rows, at::kBFloat16, "rows");
    check_fm(dX0, local_col, w_local, labels, coef, metrics);
    check(rows.dim() == 2, "rows [R, D]");
    const int D = (int)rows.size(1);
    check(D == 8 || D == 16 || D == 32, "row gather: D in {8, 16, 32}");
    check(S > 0 && S <= 64, "1..64 keys per example");
    check(dX0.numel() >= B * S * D, "dX0 too small");
    const int64_t* ip = optr<int64_t>(idx, at::kLong, "idx");
    const FmArgs a = check_fm_sizes(local_col, labels, coef, metrics, vals, hist, B, S, nbins);
    psamd::fm_fwd_bwd(nullptr, rows.data_ptr(), ip, ip ? idx->numel() : 0, rows.size(0), a.v, B, S,
                      D, ptr<int32_t>(local_col), ptr<float>(w_local), w_local.numel(),
                      ptr<float>(labels), ptr<float>(coef), dX0.data_ptr(), ptr<double>(metrics),
                      a.h, nbins, acc_stripes_of(metrics), cur_stream());
  });
  m.def("fm_l2", [](Tensor dE, Tensor rows, optional<Tensor> idx, optional<Tensor> n_dev,
                    int64_t u_cap, double lambda) {
    chk(dE, at::kFloat, "dE");
    chk(rows, at::kBFloat16, "rows");
    check(rows.dim() == 2, "rows [n, D]");
    const int D = (int)rows.size(1);
    check(dE.numel() >= u_cap * D, "dE too small");
    const int64_t* ip = optr<int64_t>(idx, at::kLong, "idx");
    if (ip) check(idx->numel() >= u_cap, "idx too small");
    else check(rows.size(0) >= u_cap, "rows too small");
    psamd::fm_l2(ptr<float>(dE), rows.data_ptr(), ip, rows.size(0),
                 optr<int32_t>(n_dev, at::kInt, "n_dev"), u_cap, D, (float)lambda, cur_stream());
  });
}
