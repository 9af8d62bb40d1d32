// Bindings of the tp / tpf kernel family (launchers: tploc.h): the tile localiser
// (tploc.hip, tploc_bucket.hip), the flat one (tploc_flat.hip), the fused forward / backward
// (tploc_fused.hip) and the fused step and flat exchange (tploc_step.hip).
#include "bind_common.h"
#include "countmin.cuh"
#include "tploc.h"

using namespace psamd_bind;

namespace {

Launch make_tp_seg_update(Tensor pos_s, Tensor segid, int64_t n, Tensor n_ent, Tensor psum,
                          Tensor seg_start, Tensor n_uniq, Tensor pieces, Tensor slot_idx,
                          Tensor slots, int algo, int lr_type, double alpha, double beta,
                          double l1, double l2, double grad_scale, double max_delta,
                          optional<Tensor> stats, optional<Tensor> hist, optional<Tensor> metrics,
                          optional<Tensor> step_counter) {
  chk(pos_s, at::kInt, "pos_s");
  chk(segid, at::kInt, "segid");
  chk(n_ent, at::kInt, "n_ent");
  chk(psum, at::kFloat, "psum");
  chk(seg_start, at::kInt, "seg_start");
  chk(n_uniq, at::kInt, "n_uniq");
  chk(pieces, at::kLong, "pieces");
  chk(slot_idx, at::kLong, "slot_idx");
  const int64_t cap = slot_capacity(slots);
  check(n > 0, "tp_seg_update: n > 0");
  check(alpha > 0, "learning rate alpha must be > 0");
  const int64_t N = psamd::tploc_stride(n);
  check(pos_s.numel() >= N && segid.numel() >= N && psum.numel() >= N &&
            seg_start.numel() >= N + 1, "tp_seg_update: entry buffers < stride");
  const int64_t ucap = std::min(pieces.numel(), slot_idx.numel());
  psamd::AucOut auc = auc_out(
      hist, metrics, "tp_seg_update: hist = stripes x 2 x 2048 (<= 8 stripes) with metrics");
  const psamd::StripedAcc acc = striped_acc(stats, "stats");
  auc.step_counter = step_counter_of(step_counter);
  const psamd::UpdateParams p =
      update_params(algo, lr_type, alpha, beta, l1, l2, grad_scale, max_delta);
  return [=, keep = std::vector<optional<Tensor>>{pos_s, segid, n_ent, psum, seg_start, n_uniq,
                                                  pieces, slot_idx, slots, stats, hist, metrics,
                                                  step_counter}](hipStream_t st) {
    psamd::tp_seg_update(ptr<int32_t>(pos_s), ptr<int32_t>(segid), n, ptr<int32_t>(n_ent),
                         ptr<float>(psum), ptr<int32_t>(seg_start), ptr<int32_t>(n_uniq),
                         reinterpret_cast<unsigned long long*>(pieces.data_ptr()), ucap,
                         ptr<int64_t>(slot_idx), slots.data_ptr(), cap, p, acc, auc, st);
  };
}

// What the two fused forward / backward launchers share: the buffers of one localisation
// checked against the geometry of n keys, and the optional outputs. `op` prefixes the
// messages; csc_always: the entry CSC buffers are needed even without the reduce;
// check_rows: the op's own check of its row layout, run after the dtype checks.
struct FwdBwd {
  const int32_t* eu;
  int32_t *ps, *sg, *ne;
  float* gr;
  const float* v;
  uint32_t* hp;
  double* mp;
  int mstripes, hstripes;
  int64_t gcap;
};
template <typename RowCheck>
FwdBwd check_fwd_bwd(const std::string& op, bool csc_always, RowCheck check_rows,
                     const Tensor& rep, const Tensor& dcnt, const optional<Tensor>& ent_uid, int64_t n,
                     const optional<Tensor>& vals, const Tensor& w_local, const Tensor& labels,
                     int64_t B, const Tensor& coef, const optional<Tensor>& metrics,
                     const optional<Tensor>& hist, int nbins, const Tensor& psum,
                     const optional<Tensor>& pos_s, const optional<Tensor>& segid,
                     const optional<Tensor>& n_ent, const optional<Tensor>& grad, bool reduce) {
  FwdBwd f;
  f.eu = optr<int32_t>(ent_uid, at::kInt, "ent_uid");
  chk(w_local, at::kFloat, "w_local");
  chk(labels, at::kFloat, "labels");
  chk(coef, at::kFloat, "coef");
  chk(psum, at::kFloat, "psum");
  f.ps = optr<int32_t>(pos_s, at::kInt, "pos_s");
  f.sg = optr<int32_t>(segid, at::kInt, "segid");
  f.ne = optr<int32_t>(n_ent, at::kInt, "n_ent");
  f.gr = optr<float>(grad, at::kFloat, "grad");
  check_rows();
  const int64_t N = f.eu ? psamd::tploc_stride(n) : psamd::tpf_stride(n);
  check(rep.numel() >= n && dcnt.numel() >= N / psamd::tploc_tile(), op + ": rep / dcnt");
  check(psum.numel() >= N, op + ": psum < stride");
  if (f.eu) {
    check(ent_uid->numel() >= N, op + ": ent_uid < stride");
    check((!csc_always && !reduce) || (f.ps && f.sg && f.ne && f.gr && pos_s->numel() >= N &&
                                       segid->numel() >= N),
          op + ": entry CSC buffers");
  } else {
    check(w_local.numel() >= N && !reduce, op + " flat: w_ent >= stride, no reduce");
  }
  check(labels.numel() >= B && coef.numel() >= B, "labels/coef too small");
  f.v = optr<float>(vals, at::kFloat, "vals");
  if (f.v) check(vals->numel() >= n, "vals too small");
  f.hp = optr<uint32_t>(hist, at::kInt, "hist");
  if (f.hp) check(nbins > 0 && nbins <= 8192 && hist->numel() >= 2 * nbins, "hist size");
  f.mp = optr<double>(metrics, at::kDouble, "metrics");
  if (f.mp) check(metrics->numel() >= 5, "metrics needs >= 5 slots");
  f.mstripes = acc_stripes_of(metrics);
  f.hstripes = f.hp ? (int)std::max<int64_t>(1, hist->numel() / (2 * nbins)) : 1;
  f.gcap = f.gr ? grad->numel() : 0;
  return f;
}

// ent_uid = None: the flat layout (w_local = w_ent in tile-entry order, no entry CSC;
// pos_s / segid / n_ent / grad unused and reduce must be false)
Launch make_tp_fwd_bwd(Tensor rep, Tensor dcnt, optional<Tensor> ent_uid, int64_t n, int width,
                       optional<Tensor> vals, Tensor w_local, Tensor labels, int64_t B,
                       int loss_type, Tensor coef, optional<Tensor> metrics,
                       optional<Tensor> hist, int nbins, Tensor psum, optional<Tensor> pos_s,
                       optional<Tensor> segid, optional<Tensor> n_ent, optional<Tensor> grad,
                       bool reduce) {
  chk(rep, at::kShort, "rep");
  chk(dcnt, at::kInt, "dcnt");
  auto check_rows = [&] {
    check(psamd::tp_fwd_bwd_supported(width) && n == B * (int64_t)width && n > 0,
          "tp_fwd_bwd: fixed width 9..64 (tp_fwd_bwd_supported) and n == B * width");
  };
  const FwdBwd f = check_fwd_bwd("tp_fwd_bwd", true, check_rows, rep, dcnt, ent_uid, n, vals,
                                 w_local, labels, B, coef, metrics, hist, nbins, psum, pos_s,
                                 segid, n_ent, grad, reduce);
  return [=, keep = std::vector<optional<Tensor>>{rep, dcnt, ent_uid, vals, w_local, labels, coef,
                                                  metrics, hist, psum, pos_s, segid, n_ent,
                                                  grad}](hipStream_t st) {
    psamd::tp_fwd_bwd(ptr<uint16_t>(rep), ptr<int32_t>(dcnt), f.eu, n, width, f.v,
                      ptr<float>(w_local), w_local.numel(), ptr<float>(labels), B, loss_type,
                      ptr<float>(coef), f.mp, f.hp, nbins, f.mstripes, f.hstripes,
                      ptr<float>(psum), f.ps, f.sg, f.ne, f.gr, f.gcap, reduce, st);
  };
}

// Variable-width / valued rows (CSR): row_ptr [B+1] int64, rows [n] int32 (row of every
// occurrence, csr_rows), vals [n] or None. Same buffers / flat rule as make_tp_fwd_bwd.
Launch make_tp_fwd_bwd_csr(Tensor rep, Tensor dcnt, optional<Tensor> ent_uid, int64_t n,
                           Tensor row_ptr, Tensor rows, optional<Tensor> vals, Tensor w_local,
                           Tensor labels, int64_t B, int loss_type, Tensor coef,
                           optional<Tensor> metrics, optional<Tensor> hist, int nbins,
                           Tensor psum, optional<Tensor> pos_s, optional<Tensor> segid,
                           optional<Tensor> n_ent, optional<Tensor> grad, bool reduce) {
  chk(rep, at::kShort, "rep");
  chk(dcnt, at::kInt, "dcnt");
  chk(row_ptr, at::kLong, "row_ptr");
  chk(rows, at::kInt, "rows");
  auto check_rows = [&] {
    check(n > 0 && B > 0 && row_ptr.numel() >= B + 1 && rows.numel() >= n,
          "tp_fwd_bwd_csr: row_ptr [B+1], rows [n]");
    check(psamd::tploc_stride(n) / psamd::tploc_tile() <= 640, "tp_fwd_bwd_csr: <= 5.2 M keys");
  };
  const FwdBwd f = check_fwd_bwd("tp_fwd_bwd_csr", false, check_rows, rep, dcnt, ent_uid, n, vals,
                                 w_local, labels, B, coef, metrics, hist, nbins, psum, pos_s,
                                 segid, n_ent, grad, reduce);
  return [=, keep = std::vector<optional<Tensor>>{rep, dcnt, ent_uid, row_ptr, rows, vals,
                                                  w_local, labels, coef, metrics, hist, psum,
                                                  pos_s, segid, n_ent, grad}](hipStream_t st) {
    psamd::tp_fwd_bwd_csr(ptr<uint16_t>(rep), ptr<int32_t>(dcnt), f.eu, n, ptr<int64_t>(row_ptr),
                          ptr<int32_t>(rows), f.v, ptr<float>(w_local), w_local.numel(),
                          ptr<float>(labels), B, loss_type, ptr<float>(coef), f.mp, f.hp, nbins,
                          f.mstripes, f.hstripes, ptr<float>(psum), f.ps, f.sg, f.ne, f.gr,
                          f.gcap, reduce, st);
  };
}

// Flat-layout buffers of one localisation (Localizer mode "tpf"): checked against the
// geometry of an n-key minibatch.
struct TpfBufs {
  Tensor cnt, uniqf, ent_pos, ent_j, slot_u;
};
// (partial = true: empty tensors are buffers the caller does not use)
void check_tpf(const TpfBufs& f, int64_t n, int bits, const char* what, bool partial = false) {
  check(psamd::tploc_supported(n, bits), std::string(what) + ": tp geometry (2..34 key bits)");
  const int64_t g = psamd::tpf_groups(n, bits);
  auto need = [&](const Tensor& t, at::ScalarType dt, const char* name, int64_t m) {
    if (partial && t.numel() == 0) return;
    chk(t, dt, name);
    check(t.numel() >= m, std::string(what) + ": " + name + " smaller than the geometry");
  };
  need(f.cnt, at::kInt, "cnt", 4 * g);
  need(f.uniqf, at::kLong, "uniqf", g * psamd::tpf_key_region());
  need(f.ent_pos, at::kInt, "ent_pos", g * psamd::tpf_entry_region());
  need(f.ent_j, at::kShort, "ent_j", g * psamd::tpf_entry_region());
  need(f.slot_u, at::kInt, "slot_u", g * psamd::tpf_key_region());
}

// filt (the fused tail filter, tploc_flat.hip tpf_filter_unit): (cells int32 [the sketch's
// byte cells as words], rsize, rshift, k, vmax, freq, ecnt uint8 [>= tpf_stride_max(n)],
// w_ent float32 [the FlatLoc's tile-entry weights][, cnt_pre int32 [like cnt]: the
// unfiltered counts])
Launch make_localize_tpf(Tensor keys, int64_t n, int bits, Tensor temp, Tensor dcnt, Tensor rep,
                         Tensor uniqf, Tensor ent_pos, Tensor ent_j, Tensor cnt, Tensor err,
                         bool sorted, optional<py::tuple> filt, int stage) {
  check(stage >= 0 && stage <= 4,
        "localize_tpf: stage 0 (all), 1 (tile), 2 (bucket), 3 (tail filter), 4 (tile + bucket)");
  chk(keys, at::kLong, "keys");
  chk(temp, at::kByte, "temp");
  chk(dcnt, at::kInt, "dcnt");
  chk(rep, at::kShort, "rep");
  chk(err, at::kInt, "err");
  check(n > 0 && keys.numel() >= n, "localize_tpf: n keys");
  check_tpf(TpfBufs{cnt, uniqf, ent_pos, ent_j, ent_pos}, n, bits, "localize_tpf");
  const int64_t T = psamd::tpf_stride(n) / psamd::tploc_tile();
  check(dcnt.numel() >= T && rep.numel() >= n, "localize_tpf: dcnt / rep");
  check((size_t)temp.numel() >= psamd::tpf_temp_bytes(n, bits), "localize_tpf: temp too small");
  const psamd::KeyMix km = make_keymix(bits);
  std::vector<Tensor> keep{keys, temp, dcnt, rep, uniqf, ent_pos, ent_j, cnt, err};
  bool has_f = false;
  psamd::CmArgs ca{};
  Tensor ecnt, w_ent, cnt_pre;
  if (filt && !filt->is_none()) {
    const py::tuple& f = *filt;
    check(f.size() == 8 || f.size() == 9,
          "localize_tpf filt: (cells, rsize, rshift, k, vmax, freq, ecnt, w_ent[, cnt_pre])");
    if (f.size() == 9 && !f[8].is_none()) {
      cnt_pre = f[8].cast<Tensor>();
      chk(cnt_pre, at::kInt, "filt cnt_pre");
      check(cnt_pre.numel() >= cnt.numel(), "localize_tpf filt: cnt_pre smaller than cnt");
      keep.push_back(cnt_pre);
    }
    Tensor cells = f[0].cast<Tensor>();
    ecnt = f[6].cast<Tensor>();
    w_ent = f[7].cast<Tensor>();
    chk(cells, at::kInt, "filt cells");
    chk(ecnt, at::kByte, "filt ecnt");
    chk(w_ent, at::kFloat, "filt w_ent");
    ca.rsize = f[1].cast<uint64_t>();
    ca.rshift = f[2].cast<int>();
    ca.k = f[3].cast<int>();
    ca.vmax = f[4].cast<uint32_t>();
    ca.freq = f[5].cast<int>();
    check(ca.k >= 1 && ca.k <= 30 && ca.vmax >= 1 && ca.vmax <= 255 && ca.freq >= 0 &&
              ca.freq < 255,
          "localize_tpf filt: k / vmax / freq");
    check(ca.rsize > 0 && ca.rsize % 64 == 0 && ca.rshift >= 0 && ca.rshift <= bits &&
              bits - ca.rshift <= 30 &&
              (ca.rsize << (bits - ca.rshift)) <= (uint64_t)cells.numel() * 4,
          "localize_tpf filt: sketch regions exceed the cells");
    check(ecnt.numel() >= psamd::tpf_stride_max(n), "localize_tpf filt: ecnt too small");
    check(w_ent.numel() >= psamd::tpf_stride(n), "localize_tpf filt: w_ent too small");
    ca.cells = ptr<uint32_t>(cells);
    ca.ncells32 = (uint64_t)cells.numel() * 4 <= ((uint64_t)1 << 32) ? 1 : 0;
    keep.push_back(cells);
    keep.push_back(ecnt);
    keep.push_back(w_ent);
    has_f = true;
  }
  return [=, keep = std::move(keep)](hipStream_t st) {
    psamd::localize_tpf(ptr<uint64_t>(keys), n, km, temp.data_ptr(), (size_t)temp.numel(),
                        ptr<int32_t>(dcnt), ptr<uint16_t>(rep), ptr<uint64_t>(uniqf),
                        ptr<int32_t>(ent_pos), ptr<uint16_t>(ent_j), ptr<int32_t>(cnt),
                        ptr<int32_t>(err), sorted, st, has_f ? &ca : nullptr,
                        has_f ? ptr<uint8_t>(ecnt) : nullptr, has_f ? ptr<float>(w_ent) : nullptr,
                        has_f ? w_ent.numel() : 0,
                        cnt_pre.defined() ? ptr<int32_t>(cnt_pre) : nullptr, stage);
  };
}

// (cnt, uniqf, ent_pos, ent_j, slot_u) from Python
optional<TpfBufs> tpf_bufs(const optional<py::tuple>& t) {
  if (!t.has_value() || t->is_none()) return c10::nullopt;
  check(t->size() == 5, "flat buffers: (cnt, uniqf, ent_pos, ent_j, slot_u)");
  return TpfBufs{(*t)[0].cast<Tensor>(), (*t)[1].cast<Tensor>(), (*t)[2].cast<Tensor>(),
                 (*t)[3].cast<Tensor>(), (*t)[4].cast<Tensor>()};
}

// The flat step boundary: update A (optional) then pull B (optional), same n.
Launch make_tpf_step(int64_t n, int bits, optional<py::tuple> A_, optional<Tensor> psum,
                     optional<py::tuple> B_, optional<Tensor> w_ent, Tensor slots, int init_type,
                     double init_v, double init_s, uint64_t seed, optional<Tensor> err,
                     optional<Tensor> inserted, uint64_t home_base, uint64_t home_m, int algo,
                     int lr_type, double alpha, double beta, double l1, double l2,
                     double grad_scale, double max_delta, optional<Tensor> stats,
                     optional<Tensor> hist, optional<Tensor> metrics,
                     optional<Tensor> step_counter) {
  const optional<TpfBufs> A = tpf_bufs(A_), B = tpf_bufs(B_);
  const psamd::TableRef t = table_ref(slots, home_base, home_m);
  check(t.cap <= ((int64_t)1 << 32), "tpf_step: u32 slot ids need <= 2^32 slots");
  check(A.has_value() || B.has_value(), "tpf_step: nothing to do");
  check(alpha > 0, "learning rate alpha must be > 0");
  const int64_t N = psamd::tpf_stride(n);
  if (A) {
    check_tpf(*A, n, bits, "tpf_step A");
    check(psum.has_value(), "tpf_step: update needs psum");
    chk(*psum, at::kFloat, "psum");
    check(psum->numel() >= N, "tpf_step: psum < stride");
  }
  if (B) {
    check_tpf(*B, n, bits, "tpf_step B");
    check(w_ent.has_value(), "tpf_step: pull needs w_ent");
    chk(*w_ent, at::kFloat, "w_ent");
    check(w_ent->numel() >= N, "tpf_step: w_ent < stride");
  }
  psamd::AucOut auc = auc_out(
      hist, metrics, "tpf_step: hist = stripes x 2 x 2048 (<= 8 stripes) with metrics");
  const psamd::StripedAcc acc = striped_acc(stats, "stats");
  auc.step_counter = step_counter_of(step_counter);
  const psamd::KeyInit init = key_init(init_type, init_v, init_s, seed);
  const psamd::UpdateParams p =
      update_params(algo, lr_type, alpha, beta, l1, l2, grad_scale, max_delta);
  int32_t* ep = optr<int32_t>(err, at::kInt, "err");
  int32_t* ip = optr<int32_t>(inserted, at::kInt, "inserted");
  std::vector<optional<Tensor>> keep{psum, w_ent, slots, err, inserted, stats, hist, metrics,
                                     step_counter};
  for (const auto* f : {A ? &*A : nullptr, B ? &*B : nullptr})
    if (f) keep.insert(keep.end(), {f->cnt, f->uniqf, f->ent_pos, f->ent_j, f->slot_u});
  const TpfBufs* a = A ? &*A : nullptr;
  const TpfBufs* b = B ? &*B : nullptr;
  auto p32 = [](const TpfBufs* f, Tensor TpfBufs::*m) -> int32_t* {
    return f ? reinterpret_cast<int32_t*>((f->*m).data_ptr()) : nullptr;
  };
  int32_t *ca = p32(a, &TpfBufs::cnt), *pa = p32(a, &TpfBufs::ent_pos);
  uint16_t* ja = reinterpret_cast<uint16_t*>(p32(a, &TpfBufs::ent_j));
  uint32_t* sa = reinterpret_cast<uint32_t*>(p32(a, &TpfBufs::slot_u));
  int32_t *cb = p32(b, &TpfBufs::cnt), *pb = p32(b, &TpfBufs::ent_pos);
  uint16_t* jb = reinterpret_cast<uint16_t*>(p32(b, &TpfBufs::ent_j));
  uint32_t* sb = reinterpret_cast<uint32_t*>(p32(b, &TpfBufs::slot_u));
  uint64_t* ub = reinterpret_cast<uint64_t*>(p32(b, &TpfBufs::uniqf));
  float* ps = A ? ptr<float>(*psum) : nullptr;
  float* we = B ? ptr<float>(*w_ent) : nullptr;
  const int64_t pcap = A ? psum->numel() : 0, wcap = B ? w_ent->numel() : 0;
  return [=](hipStream_t st) {
    (void)keep;
    psamd::tpf_step(n, bits, ca, pa, ja, sa, ps, pcap, cb, ub, pb, jb, sb, we, wcap, t, init, ep,
                    ip, p, acc, auc, st);
  };
}

}  // namespace

void psamd_bind::register_tploc(py::module_& m) {
  // ------ tile dedup + bucket partition localisation (tploc.hip; fused: tploc_fused.hip) ------
  m.def("tploc_stride", [](int64_t n) { return psamd::tploc_stride(n); });
  // flat layout: entry stride of n keys / bound over minibatches of <= n keys / log2 tile
  m.def("tpf_stride", [](int64_t n) { return psamd::tpf_stride(n); });
  m.def("tpf_stride_max", [](int64_t n) { return psamd::tpf_stride_max(n); });
  m.def("tpf_tile_log2", [](int64_t n) { return psamd::tpf_tile_log2(n); });
  m.def("tploc_buckets", [](int64_t n, int bits) { return psamd::tploc_buckets(n, bits); });
  m.def("tploc_supported", [](int64_t n, int bits) { return psamd::tploc_supported(n, bits); });
  m.def("tploc_temp_bytes", [](int64_t n, int bits) { return (int64_t)psamd::tploc_temp_bytes(n, bits); });
  m.def("localize_tp", [](Tensor keys, int bits, Tensor temp, Tensor dcnt, Tensor rep, Tensor pos_s,
                          Tensor segid, Tensor uniq, Tensor seg_start, Tensor ent_uid,
                          optional<Tensor> local_col, Tensor n_uniq, Tensor n_ent, Tensor grad,
                          optional<Tensor> pieces, Tensor err, optional<Tensor> prof) {
    chk(keys, at::kLong, "keys");
    chk(temp, at::kByte, "temp");
    chk(dcnt, at::kInt, "dcnt");
    chk(rep, at::kShort, "rep");
    chk(pos_s, at::kInt, "pos_s");
    chk(segid, at::kInt, "segid");
    chk(uniq, at::kLong, "uniq");
    chk(seg_start, at::kInt, "seg_start");
    chk(ent_uid, at::kInt, "ent_uid");
    int32_t* lc = optr<int32_t>(local_col, at::kInt, "local_col");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(n_ent, at::kInt, "n_ent");
    chk(grad, at::kFloat, "grad");
    chk(err, at::kInt, "err");
    const int64_t n = keys.numel();
    check(psamd::tploc_supported(n, bits), "tp localisation: 2..34 key bits, n <= 5.2M");
    if (lc) check(local_col->numel() >= n, "local_col too small");
    const int64_t N = psamd::tploc_stride(n);
    const int64_t T = N / psamd::tploc_tile();
    check(pos_s.numel() >= N && segid.numel() >= N && uniq.numel() >= N &&
              seg_start.numel() >= N + 1 && ent_uid.numel() >= N && grad.numel() >= N,
          "tp localisation buffers < stride");
    check(dcnt.numel() >= T && rep.numel() >= n, "tp buffers too small");
    check((size_t)temp.numel() >= psamd::tploc_temp_bytes(n, bits), "tp temp too small");
    psamd::localize_tp(ptr<uint64_t>(keys), n, make_keymix(bits), temp.data_ptr(),
                       (size_t)temp.numel(), ptr<int32_t>(dcnt), ptr<uint16_t>(rep),
                       ptr<int32_t>(pos_s), ptr<int32_t>(segid), ptr<uint64_t>(uniq),
                       ptr<int32_t>(seg_start), ptr<int32_t>(ent_uid), lc,
                       ptr<int32_t>(n_uniq), ptr<int32_t>(n_ent), ptr<float>(grad),
                       reinterpret_cast<unsigned long long*>(optr<int64_t>(pieces, at::kLong, "pieces")),
                       ptr<int32_t>(err), uniq.numel(),
                       reinterpret_cast<uint64_t*>(optr<int64_t>(prof, at::kLong, "prof")),
                       cur_stream());
  });
  m.def("tp_backward", [](Tensor rep, Tensor dcnt, int64_t n, optional<Tensor> rows, int width,
                          optional<Tensor> vals, Tensor coef, Tensor psum, Tensor pos_s,
                          Tensor segid, Tensor n_ent, Tensor grad) {
    chk(rep, at::kShort, "rep");
    chk(dcnt, at::kInt, "dcnt");
    chk(coef, at::kFloat, "coef");
    chk(psum, at::kFloat, "psum");
    chk(pos_s, at::kInt, "pos_s");
    chk(segid, at::kInt, "segid");
    chk(n_ent, at::kInt, "n_ent");
    chk(grad, at::kFloat, "grad");
    const int64_t N = psamd::tploc_stride(n);
    check(n > 0 && rep.numel() >= n && dcnt.numel() >= N / psamd::tploc_tile(), "tp backward: rep / dcnt");
    check(psum.numel() >= N && pos_s.numel() >= N && segid.numel() >= N, "tp backward buffers");
    const int32_t* r = optr<int32_t>(rows, at::kInt, "rows");
    if (r) check(rows->numel() >= n, "rows too small");
    else check(width > 0, "width must be > 0 without rows");
    const float* v = optr<float>(vals, at::kFloat, "vals");
    if (v) check(vals->numel() >= n, "vals too small");
    psamd::tp_backward(ptr<uint16_t>(rep), ptr<int32_t>(dcnt), n, r, width, v, ptr<float>(coef),
                       coef.numel(), ptr<float>(psum), ptr<int32_t>(pos_s), ptr<int32_t>(segid),
                       ptr<int32_t>(n_ent), ptr<float>(grad), grad.numel(), cur_stream());
  });
  def_launch(m, "tp_seg_update", make_tp_seg_update);
  m.def("tp_gather", [](Tensor rep, Tensor ent_uid, int64_t n, Tensor local_col) {
    chk(rep, at::kShort, "rep");
    chk(ent_uid, at::kInt, "ent_uid");
    chk(local_col, at::kInt, "local_col");
    check(n > 0 && rep.numel() >= n && local_col.numel() >= n &&
              ent_uid.numel() >= psamd::tploc_stride(n), "tp gather buffers");
    psamd::tp_gather(ptr<uint16_t>(rep), ptr<int32_t>(ent_uid), n, ptr<int32_t>(local_col),
                     cur_stream());
  });
  m.def("tp_fwd_bwd_supported", [](int width) { return psamd::tp_fwd_bwd_supported(width); });
  // ---- flat 1-GPU layout ("tpf": tploc_bucket.hip, tploc_flat.hip, tploc_step.hip)
  m.def("tpf_groups", [](int64_t n, int bits) { return psamd::tpf_groups(n, bits); });
  m.def("tpf_key_region", []() { return psamd::tpf_key_region(); });
  m.def("tpf_entry_region", []() { return psamd::tpf_entry_region(); });
  // the logical bucket group of physical block bid (tploc.cuh tpf_xcd_group_of), host side
  m.def("tpf_xcd_group", [](int bid, int groups) {
    check(groups >= 1 && bid >= 0 && bid < groups, "tpf_xcd_group: 0 <= bid < groups");
    return psamd::tpf_xcd_group(bid, groups);
  });
  m.def("tpf_temp_bytes", [](int64_t n, int bits) { return psamd::tpf_temp_bytes(n, bits); });
  // (the Python API is fixed: the eager op takes n from keys, the list op takes it)
  m.def("localize_tpf", [](Tensor keys, int bits, Tensor temp, Tensor dcnt, Tensor rep,
                           Tensor uniqf, Tensor ent_pos, Tensor ent_j, Tensor cnt, Tensor err,
                           bool sorted, optional<py::tuple> filt, int stage) {
    make_localize_tpf(keys, keys.numel(), bits, temp, dcnt, rep, uniqf, ent_pos, ent_j, cnt,
                      err, sorted, filt, stage)(cur_stream());
  }, py::arg("keys"), py::arg("bits"), py::arg("temp"), py::arg("dcnt"), py::arg("rep"),
     py::arg("uniqf"), py::arg("ent_pos"), py::arg("ent_j"), py::arg("cnt"), py::arg("err"),
     py::arg("sorted"), py::arg("filt") = py::none(), py::arg("stage") = 0);
  launch_list_class(m).def("add_localize_tpf", [](LaunchList& l, Tensor keys, int64_t n, int bits,
                                                  Tensor temp, Tensor dcnt, Tensor rep,
                                                  Tensor uniqf, Tensor ent_pos, Tensor ent_j,
                                                  Tensor cnt, Tensor err, bool sorted,
                                                  optional<py::tuple> filt, int stage) {
    l.push(make_localize_tpf(keys, n, bits, temp, dcnt, rep, uniqf, ent_pos, ent_j, cnt, err,
                             sorted, filt, stage), "localize_tpf");
  }, py::arg("keys"), py::arg("n"), py::arg("bits"), py::arg("temp"), py::arg("dcnt"),
     py::arg("rep"), py::arg("uniqf"), py::arg("ent_pos"), py::arg("ent_j"), py::arg("cnt"),
     py::arg("err"), py::arg("sorted"), py::arg("filt") = py::none(), py::arg("stage") = 0);
  // ---- the padded multi-GPU exchange on the flat layout (rows as in exchange.hip)
  m.def("tpf_exchange_ok", [](int64_t n, int bits, int G) {
    return psamd::tpf_exchange_ok(n, bits, G);
  });
  m.def("tpf_pack_keys", [](int64_t n, int bits, int G, Tensor cnt, Tensor uniqf, int64_t C, int kw,
                            int64_t H, Tensor send, optional<Tensor> ovf) {
    check_tpf(TpfBufs{cnt, uniqf, cnt.new_empty({0}, at::kInt), cnt.new_empty({0}, at::kShort),
                      cnt.new_empty({0}, at::kInt)}, n, bits, "tpf_pack_keys", true);
    chk(send, at::kInt, "send");
    check(psamd::tpf_exchange_ok(n, bits, G), "tpf_pack_keys: G a power of two dividing groups");
    check((kw == 1 || kw == 2) && C > 0 && H >= 4 + C * kw + 1 && send.numel() >= G * H,
          "tpf_pack_keys: row geometry");
    psamd::tpf_pack_keys(n, bits, G, ptr<int32_t>(cnt), ptr<uint64_t>(uniqf), C, kw, H,
                         ptr<int32_t>(send), optr<int32_t>(ovf, at::kInt, "ovf"), cur_stream());
  }, py::arg("n"), py::arg("bits"), py::arg("G"), py::arg("cnt"), py::arg("uniqf"), py::arg("C"),
     py::arg("kw"), py::arg("H"), py::arg("send"), py::arg("ovf"));
  m.def("tpf_unpack_w", [](int64_t n, int bits, int G, Tensor cnt, Tensor ent_pos, Tensor ent_j,
                           int64_t C, Tensor wrecv, Tensor w_ent, int64_t wstride) {
    // wstride: row stride of wrecv (0 = C; the merged exchange reads the weights in
    // place from the received rows)
    const int64_t ws = wstride > 0 ? wstride : C;
    check_tpf(TpfBufs{cnt, cnt.new_empty({0}, at::kLong), ent_pos, ent_j,
                      cnt.new_empty({0}, at::kInt)}, n, bits, "tpf_unpack_w", true);
    chk(wrecv, at::kFloat, "wrecv");
    chk(w_ent, at::kFloat, "w_ent");
    check(psamd::tpf_exchange_ok(n, bits, G), "tpf_unpack_w: G a power of two dividing groups");
    check(C > 0 && ws >= C && wrecv.numel() >= (G - 1) * ws + C &&
          w_ent.numel() >= psamd::tpf_stride(n), "tpf_unpack_w: buffers");
    psamd::tpf_unpack_w(n, bits, G, ptr<int32_t>(cnt), ptr<int32_t>(ent_pos),
                        ptr<uint16_t>(ent_j), C, ptr<float>(wrecv), ws, ptr<float>(w_ent),
                        w_ent.numel(), cur_stream());
  }, py::arg("n"), py::arg("bits"), py::arg("G"), py::arg("cnt"), py::arg("ent_pos"),
     py::arg("ent_j"), py::arg("C"), py::arg("wrecv"), py::arg("w_ent"), py::arg("wstride") = 0);
  m.def("tpf_pack_grads", [](int64_t n, int bits, int G, Tensor cnt, Tensor ent_pos, Tensor ent_j,
                             int64_t C, int kw, int64_t H, Tensor psum, Tensor send,
                             optional<Tensor> gstage, optional<Tensor> hist,
                             optional<Tensor> metrics, optional<Tensor> step_counter,
                             optional<Tensor> ovf, optional<Tensor> ovf_host) {
    check_tpf(TpfBufs{cnt, cnt.new_empty({0}, at::kLong), ent_pos, ent_j,
                      cnt.new_empty({0}, at::kInt)}, n, bits, "tpf_pack_grads", true);
    chk(psum, at::kFloat, "psum");
    chk(send, at::kInt, "send");
    check(psamd::tpf_exchange_ok(n, bits, G), "tpf_pack_grads: G a power of two dividing groups");
    check((kw == 1 || kw == 2) && C > 0 && H >= 4 + C * kw + 1 && send.numel() >= G * H,
          "tpf_pack_grads: row geometry");
    check(psum.numel() >= psamd::tpf_stride(n), "tpf_pack_grads: psum < stride");
    float* gs = optr<float>(gstage, at::kFloat, "gstage");
    if (gs)  // (+ 2 floats per bucket group: the workgroups' min / max partials)
      check(gstage->numel() >= G * C + 2 * (int64_t)psamd::tpf_groups(n, bits),
            "tpf_pack_grads: gstage < G * C + 2 * groups");
    else check(H >= 4 + C * kw + C, "tpf_pack_grads: f32 gradient rows");
    psamd::AucOut auc =
        auc_out(hist, metrics, "tpf_pack_grads: hist = stripes x 2 x 2048 with metrics");
    int32_t* op = optr<int32_t>(ovf, at::kInt, "ovf");
    int32_t* oh = nullptr;
    if (ovf_host.has_value() && ovf_host->defined()) {
      check(op && ovf_host->device().is_cpu() && ovf_host->is_pinned() &&
                ovf_host->scalar_type() == at::kInt,
            "ovf_host: pinned int32 host tensor (with ovf)");
      void* dptr = nullptr;
      PSAMD_HIP_CHECK(hipHostGetDevicePointer(&dptr, ovf_host->data_ptr(), 0));
      oh = reinterpret_cast<int32_t*>(dptr);
    }
    auc.step_counter = step_counter_of(step_counter);
    psamd::tpf_pack_grads(n, bits, G, ptr<int32_t>(cnt), ptr<int32_t>(ent_pos),
                          ptr<uint16_t>(ent_j), C, kw, H, ptr<float>(psum), psum.numel(),
                          ptr<int32_t>(send), gs != nullptr, gs, auc, op, oh, cur_stream());
  });
  def_launch(m, "tpf_step", make_tpf_step);
  // phase marks of the fused / the tile kernel (tuning aid): 16 int64 per tile, or None
  // to disable
  auto prof_ptr = [](const optional<Tensor>& prof) -> uint64_t* {
    if (!prof) return nullptr;
    chk(*prof, at::kLong, "prof");
    return reinterpret_cast<uint64_t*>(prof->data_ptr<int64_t>());
  };
  m.def("tp_fb_set_prof", [prof_ptr](optional<Tensor> prof) {
    psamd::tp_fb_set_prof(prof_ptr(prof));
  });
  m.def("tp_tile_set_prof", [prof_ptr](optional<Tensor> prof) {
    psamd::tp_tile_set_prof(prof_ptr(prof));
  });
  def_launch(m, "tp_fwd_bwd", make_tp_fwd_bwd);
  def_eager(m, "tp_fwd_bwd_csr", make_tp_fwd_bwd_csr);
}
