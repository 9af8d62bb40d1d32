// Bindings of the KV table (kv_table.hip), the padded exchange (exchange.hip), the
// k-value push / pull API (kvapi.hip) and the one-sided peer exchange (p2p.hip).
#include "bind_common.h"
#include "exchange.h"
#include "kv_table.h"
#include "kvapi.h"
#include "p2p.h"

using namespace psamd_bind;

namespace {

Launch make_kv_resolve(Tensor slots, Tensor keys, optional<Tensor> n_dev, Tensor out_slot,
                       optional<Tensor> out_w, bool insert, int init_type, double init_v,
                       double init_s, uint64_t seed, optional<Tensor> err,
                       optional<Tensor> inserted, uint64_t home_base, uint64_t home_m) {
  const psamd::TableRef t = table_ref(slots, home_base, home_m);
  const psamd::KeyInit init = key_init(init_type, init_v, init_s, seed);
  chk(keys, at::kLong, "keys");
  chk(out_slot, at::kLong, "out_slot");
  const int64_t n = keys.numel();
  check(out_slot.numel() >= n, "out_slot too small");
  float* w = optr<float>(out_w, at::kFloat, "out_w");
  if (w) check(out_w->numel() >= n, "out_w too small");
  int32_t* nd = optr<int32_t>(n_dev, at::kInt, "n_dev");
  int32_t* ep = optr<int32_t>(err, at::kInt, "err");
  int32_t* ip = optr<int32_t>(inserted, at::kInt, "inserted");
  // (the lambda's tensor copies keep the buffers alive as long as the launcher)
  return [=, keep = std::vector<optional<Tensor>>{slots, keys, n_dev, out_slot, out_w, err,
                                                  inserted}](hipStream_t st) {
    psamd::kv_resolve(t, ptr<uint64_t>(keys), n, nd, ptr<int64_t>(out_slot), w, insert, init, ep,
                      ip, st);
  };
}

// device-visible pointer of a pinned int32 host flag (nullptr when absent)
int32_t* host_flag(const optional<Tensor>& src, const optional<Tensor>& host_dst) {
  if (!host_dst.has_value() || !host_dst->defined()) return nullptr;
  check(src.has_value() && src->defined(), "ovf_host needs ovf");
  return pinned_word(*host_dst, "ovf_host must be a pinned int32 host tensor");
}

}  // namespace

void psamd_bind::register_table(py::module_& m) {
  // ---------------- KV table ----------------
  m.def("kv_init", [](Tensor slots) {
    psamd::kv_init(slots.data_ptr(), slot_capacity(slots), cur_stream());
  });
  def_launch(m, "kv_resolve", make_kv_resolve, py::arg("slots"), py::arg("keys"),
             py::arg("n_dev"), py::arg("out_slot"), py::arg("out_w"), py::arg("insert"),
             py::arg("init_type"), py::arg("init_v"), py::arg("init_s"), py::arg("seed"),
             py::arg("err"), py::arg("inserted"), py::arg("home_base") = 0,
             py::arg("home_m") = 0);
  m.def("kv_gather", [](Tensor slots, Tensor slot_idx, optional<Tensor> n_dev, Tensor out,
                        int field) {
    const int64_t cap = slot_capacity(slots);
    chk(slot_idx, at::kLong, "slot_idx");
    chk(out, at::kFloat, "out");
    check(field >= 0 && field < 4, "field in [0,4): w,z,n,acc");
    check(out.numel() >= slot_idx.numel(), "out too small");
    psamd::kv_gather(slots.data_ptr(), cap, ptr<int64_t>(slot_idx), slot_idx.numel(),
                     optr<int32_t>(n_dev, at::kInt, "n_dev"), ptr<float>(out), field,
                     cur_stream());
  });
  m.def("kv_set", [](Tensor slots, Tensor slot_idx, optional<Tensor> w, optional<Tensor> z,
                     optional<Tensor> nn) {
    const int64_t cap = slot_capacity(slots);
    chk(slot_idx, at::kLong, "slot_idx");
    const int64_t n = slot_idx.numel();
    for (auto* t : {&w, &z, &nn})
      if (t->has_value()) check((*t)->numel() >= n, "value array too small");
    psamd::kv_set(slots.data_ptr(), cap, ptr<int64_t>(slot_idx), n, optr<float>(w, at::kFloat, "w"),
                  optr<float>(z, at::kFloat, "z"), optr<float>(nn, at::kFloat, "n"),
                  cur_stream());
  });
  m.def("kv_update", [](Tensor slots, Tensor slot_idx, Tensor grad, optional<Tensor> n_dev,
                        int algo, int lr_type, double alpha, double beta, double l1, double l2,
                        double grad_scale, double max_delta, optional<Tensor> stats,
                        optional<Tensor> hist, optional<Tensor> metrics,
                        optional<Tensor> step_counter) {
    const int64_t cap = slot_capacity(slots);
    chk(slot_idx, at::kLong, "slot_idx");
    chk(grad, at::kFloat, "grad");
    check(grad.numel() >= slot_idx.numel(), "grad too small");
    check(alpha > 0, "learning rate alpha must be > 0");
    // optional: the step's AUC histogram -> metrics (auc_from_hist folded into block 0)
    psamd::AucOut auc = auc_out(
        hist, metrics, "kv_update: hist = stripes x 2 x 2048 (<= 8 stripes) with metrics");
    const int32_t* nd = optr<int32_t>(n_dev, at::kInt, "n_dev");
    const psamd::StripedAcc acc = striped_acc(stats, "stats");
    auc.step_counter = step_counter_of(step_counter);
    psamd::kv_update(slots.data_ptr(), cap, ptr<int64_t>(slot_idx), ptr<float>(grad),
                     slot_idx.numel(), nd,
                     update_params(algo, lr_type, alpha, beta, l1, l2, grad_scale, max_delta),
                     acc, auc, cur_stream());
  }, py::arg("slots"), py::arg("slot_idx"), py::arg("grad"), py::arg("n_dev"), py::arg("algo"),
     py::arg("lr_type"), py::arg("alpha"), py::arg("beta"), py::arg("l1"), py::arg("l2"),
     py::arg("grad_scale"), py::arg("max_delta"), py::arg("stats"), py::arg("hist") = py::none(),
     py::arg("metrics") = py::none(), py::arg("step_counter") = py::none());
  m.def("kv_accumulate", [](Tensor slots, Tensor slot_idx, Tensor grad, optional<Tensor> n_dev,
                            Tensor touched, Tensor n_touched) {
    const int64_t cap = slot_capacity(slots);
    chk(slot_idx, at::kLong, "slot_idx");
    chk(grad, at::kFloat, "grad");
    chk(touched, at::kLong, "touched");
    chk(n_touched, at::kInt, "n_touched");
    check(touched.numel() >= slot_idx.numel(), "touched buffer too small");
    psamd::kv_accumulate(slots.data_ptr(), cap, ptr<int64_t>(slot_idx), ptr<float>(grad),
                         slot_idx.numel(), optr<int32_t>(n_dev, at::kInt, "n_dev"),
                         ptr<int64_t>(touched), ptr<int32_t>(n_touched), touched.numel(),
                         cur_stream());
  });
  m.def("kv_apply_accumulated", [](Tensor slots, Tensor touched, Tensor n_touched, int algo,
                                   int lr_type, double alpha, double beta, double l1, double l2,
                                   double grad_scale, double max_delta, optional<Tensor> stats) {
    const int64_t cap = slot_capacity(slots);
    chk(touched, at::kLong, "touched");
    chk(n_touched, at::kInt, "n_touched");
    psamd::kv_apply_accumulated(
        slots.data_ptr(), cap, ptr<int64_t>(touched), ptr<int32_t>(n_touched), touched.numel(),
        update_params(algo, lr_type, alpha, beta, l1, l2, grad_scale, max_delta),
        striped_acc(stats, "stats"), cur_stream());
  });
  m.def("kv_census", [](Tensor slots) {
    const int64_t cap = slot_capacity(slots);
    auto out = torch::zeros({2}, slots.options().dtype(at::kLong));
    psamd::kv_census(slots.data_ptr(), cap, ptr<unsigned long long>(out), cur_stream());
    return out;
  });
  // warm start: (raw key, weight) pairs seeded with the optimizer state that reproduces
  // each weight; counts: the striped int64 [64 x 16] counters the launch adds to
  m.def("kv_seed", [](Tensor slots, Tensor raw, Tensor w, int bits, uint64_t lo, uint64_t last,
                      int algo, int lr_type, double alpha, double beta, double l1, double l2,
                      double n0, Tensor counts, optional<Tensor> stats, optional<Tensor> err,
                      uint64_t home_base, uint64_t home_m) {
    const psamd::TableRef t = table_ref(slots, home_base, home_m);
    chk(raw, at::kLong, "raw");
    chk(w, at::kFloat, "w");
    chk(counts, at::kLong, "counts");
    check(w.numel() >= raw.numel(), "kv_seed: fewer weights than keys");
    check(counts.numel() == psamd::kAccStripes * psamd::kAccStride,
          "kv_seed: counts must be 64 x 16 int64");
    check(alpha > 0 && n0 >= 0, "kv_seed: alpha > 0 and n0 >= 0");
    check(last >= lo, "kv_seed: empty key range");
    psamd::kv_seed(t, make_keymix(bits), ptr<uint64_t>(raw), ptr<float>(w), raw.numel(), lo,
                   last, update_params(algo, lr_type, alpha, beta, l1, l2, 1.0, 0.0), (float)n0,
                   ptr<unsigned long long>(counts), psamd::kAccStripes,
                   striped_acc(stats, "stats"), optr<int32_t>(err, at::kInt, "err"),
                   cur_stream());
  }, py::arg("slots"), py::arg("raw"), py::arg("w"), py::arg("bits"), py::arg("lo"),
     py::arg("last"), py::arg("algo"), py::arg("lr_type"), py::arg("alpha"), py::arg("beta"),
     py::arg("l1"), py::arg("l2"), py::arg("n0"), py::arg("counts"), py::arg("stats"),
     py::arg("err"), py::arg("home_base") = 0, py::arg("home_m") = 0);
  // growth: every occupied slot of `old_slots` into the larger, kv_init-ed `slots`;
  // returns the device count of slots moved (a 0-dim int64 tensor)
  m.def("kv_rehash", [](Tensor old_slots, Tensor slots, uint64_t home_base, uint64_t home_m,
                        optional<Tensor> err) {
    const int64_t old_cap = slot_capacity(old_slots);
    const psamd::TableRef t = table_ref(slots, home_base, home_m);
    check(t.cap >= old_cap, "kv_rehash: the new table must not be smaller");
    check(old_slots.device() == slots.device(), "kv_rehash: tables on different devices");
    check(old_slots.data_ptr() != slots.data_ptr(), "kv_rehash: needs a new table");
    auto moved = torch::zeros({psamd::kAccStripes * psamd::kAccStride},
                              slots.options().dtype(at::kLong));
    psamd::kv_rehash(old_slots.data_ptr(), old_cap, t, ptr<unsigned long long>(moved),
                     psamd::kAccStripes, optr<int32_t>(err, at::kInt, "err"), cur_stream());
    return moved.sum();
  }, py::arg("old_slots"), py::arg("slots"), py::arg("home_base") = 0, py::arg("home_m") = 0,
     py::arg("err") = py::none());

  // ---------------- fixed-capacity exchange (exchange.hip) ----------------
  // buffers: send/recv int32 [G * H]; row layout documented in exchange.hip
  m.def("kv_resolve_rows", [](Tensor slots, Tensor recv, int64_t H, int64_t C, int kw,
                              Tensor out_slot, Tensor out_w, bool insert, int init_type,
                              double init_v, double init_s, uint64_t seed, optional<Tensor> err,
                              optional<Tensor> inserted, uint64_t home_base, uint64_t home_m,
                              optional<Tensor> out_key, optional<Tensor> bnd, int lgP,
                              int64_t wstride) {
    const psamd::TableRef t = table_ref(slots, home_base, home_m);
    const int64_t ws = wstride > 0 ? wstride : C;
    chk(recv, at::kInt, "recv");
    chk(out_slot, at::kLong, "out_slot");
    chk(out_w, at::kFloat, "out_w");
    check(kw == 1 || kw == 2, "kw must be 1 (u32 keys) or 2 (u64 keys)");
    check(C > 0 && H >= 4 + C * kw + 1 && H % 4 == 0, "bad exchange row geometry");
    const int G = exchange_rows(recv, H, C, 4, "recv is not a whole number of rows");
    check(ws >= C && out_slot.numel() >= G * C && out_w.numel() >= (G - 1) * ws + C,
          "out_slot < G*C or out_w < (G-1)*wstride + C");
    int64_t* ok = optr<int64_t>(out_key, at::kLong, "out_key");
    if (ok) check(out_key->numel() >= G * C, "out_key < G*C");
    int32_t* bp = optr<int32_t>(bnd, at::kInt, "bnd");
    check(lgP >= 0 && lgP <= 20, "lgP in 0..20");
    if (bp) check(bnd->numel() >= G * ((1 << lgP) + 1), "bnd < G*(P+1)");
    psamd::kv_resolve_rows(t, ptr<int32_t>(recv), G, H, C, kw, ptr<int64_t>(out_slot),
                           ptr<float>(out_w), ws, insert,
                           key_init(init_type, init_v, init_s, seed),
                           optr<int32_t>(err, at::kInt, "err"),
                           optr<int32_t>(inserted, at::kInt, "inserted"),
                           reinterpret_cast<uint64_t*>(ok), bp, lgP, cur_stream());
  }, py::arg("slots"), py::arg("recv"), py::arg("H"), py::arg("C"), py::arg("kw"),
     py::arg("out_slot"), py::arg("out_w"), py::arg("insert"), py::arg("init_type"),
     py::arg("init_v"), py::arg("init_s"), py::arg("seed"), py::arg("err"), py::arg("inserted"),
     py::arg("home_base"), py::arg("home_m"), py::arg("out_key") = py::none(),
     py::arg("bnd") = py::none(), py::arg("lgP") = 0, py::arg("wstride") = 0);
  // per-push apply of every source row, partitioned by key range (see kv_apply_part_kernel)
  m.def("kv_apply_part", [](Tensor slots, Tensor slot_idx, Tensor keys, Tensor grad,
                            int64_t gstride, Tensor recv, int64_t H, int64_t C, Tensor bnd, int lgP,
                            int algo, int lr_type, double alpha, double beta, double l1, double l2,
                            double grad_scale, double max_delta, optional<Tensor> stats,
                            int ff_nb, int kw) {
    const int64_t cap = slot_capacity(slots);
    chk(slot_idx, at::kLong, "slot_idx");
    chk(keys, at::kLong, "keys");
    chk(grad, at::kFloat, "grad");
    chk(recv, at::kInt, "recv");
    chk(bnd, at::kInt, "bnd");
    const int G = exchange_rows(recv, H, C, 5);
    // ff_nb > 0: the gradients are the rows' FixingFloat codes (grad unused)
    check(ff_nb >= 0 && ff_nb <= 7 && (kw == 1 || kw == 2), "kv_apply_part: ff_nb / kw");
    if (ff_nb) check(H >= 4 + C * kw + (C * ff_nb + 3) / 4, "kv_apply_part: FixingFloat rows");
    else check_grad_rows(grad, gstride, G, C);
    check(slot_idx.numel() >= G * C && keys.numel() >= G * C, "slot_idx/keys < G*C");
    check(lgP >= 0 && lgP <= 20, "lgP in 0..20");
    check(bnd.numel() >= G * ((1 << lgP) + 1), "bnd < G*(P+1)");
    psamd::kv_apply_part(slots.data_ptr(), cap, ptr<int64_t>(slot_idx),
                         reinterpret_cast<const uint64_t*>(keys.data_ptr<int64_t>()),
                         ptr<float>(grad), gstride, ptr<int32_t>(recv), G, H, C, ptr<int32_t>(bnd),
                         lgP,
                         update_params(algo, lr_type, alpha, beta, l1, l2, grad_scale, max_delta),
                         striped_acc(stats, "stats"), ff_nb, kw, cur_stream());
  }, py::arg("slots"), py::arg("slot_idx"), py::arg("keys"), py::arg("grad"), py::arg("gstride"),
     py::arg("recv"), py::arg("H"), py::arg("C"), py::arg("bnd"), py::arg("lgP"), py::arg("algo"),
     py::arg("lr_type"), py::arg("alpha"), py::arg("beta"), py::arg("l1"), py::arg("l2"),
     py::arg("grad_scale"), py::arg("max_delta"), py::arg("stats"), py::arg("ff_nb") = 0,
     py::arg("kw") = 1);
  // aggregated pushes of every source row in one launch; grad row s at grad[s*gstride]
  m.def("kv_accumulate_rows", [](Tensor slots, Tensor slot_idx, Tensor grad, int64_t gstride,
                                 Tensor recv, int64_t H, int64_t C, Tensor touched,
                                 Tensor n_touched) {
    const int64_t cap = slot_capacity(slots);
    chk(slot_idx, at::kLong, "slot_idx");
    chk(grad, at::kFloat, "grad");
    chk(recv, at::kInt, "recv");
    chk(touched, at::kLong, "touched");
    chk(n_touched, at::kInt, "n_touched");
    const int G = exchange_rows(recv, H, C, 5);
    check_grad_rows(grad, gstride, G, C);
    check(slot_idx.numel() >= G * C, "slot_idx < G*C");
    psamd::kv_accumulate_rows(slots.data_ptr(), cap, ptr<int64_t>(slot_idx), ptr<float>(grad),
                              gstride, ptr<int32_t>(recv), G, H, C, ptr<int64_t>(touched),
                              ptr<int32_t>(n_touched), touched.numel(), cur_stream());
  });
  m.def("kv_update_rows", [](Tensor slots, Tensor slot_idx, Tensor grad, int64_t gstride,
                             Tensor recv, int64_t H, int64_t C, Tensor link, Tensor nxt, int algo,
                             int lr_type, double alpha, double beta, double l1, double l2,
                             double grad_scale, double max_delta, optional<Tensor> stats) {
    const int64_t cap = slot_capacity(slots);
    chk(slot_idx, at::kLong, "slot_idx");
    chk(grad, at::kFloat, "grad");
    chk(recv, at::kInt, "recv");
    chk(link, at::kLong, "link");
    chk(nxt, at::kInt, "nxt");
    const int G = exchange_rows(recv, H, C, 5);
    check_grad_rows(grad, gstride, G, C);
    check(slot_idx.numel() >= G * C, "slot_idx < G*C");
    check(nxt.numel() >= G * C, "nxt < G*C");
    const int64_t L = link.numel();
    check(L >= 2 * G * C && (L & (L - 1)) == 0, "link: power of two >= 2*G*C");
    psamd::kv_update_rows(slots.data_ptr(), cap, ptr<int64_t>(slot_idx), ptr<float>(grad), gstride,
                          ptr<int32_t>(recv), G, H, C,
                          reinterpret_cast<unsigned long long*>(link.data_ptr<int64_t>()), L,
                          ptr<int32_t>(nxt),
                          update_params(algo, lr_type, alpha, beta, l1, l2, grad_scale, max_delta),
                          striped_acc(stats, "stats"), cur_stream());
  });
  m.def("xchg_publish", [](Tensor src, Tensor host_dst) {
    chk(src, at::kInt, "src");
    psamd::xchg_publish(ptr<int32_t>(src),
                        pinned_word(host_dst, "host_dst must be a pinned int32 host tensor"),
                        cur_stream());
  });
  m.def("xchg_pack_keys", [](Tensor ukeys, Tensor n_uniq, Tensor off, int64_t C, int kw,
                             int64_t H, Tensor send, optional<Tensor> ovf) {
    chk(ukeys, at::kLong, "ukeys");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(off, at::kLong, "off");
    chk(send, at::kInt, "send");
    const int G = (int)off.numel() - 1;
    check(G >= 1 && G <= 64, "1..64 peers");
    check(kw == 1 || kw == 2, "kw must be 1 or 2");
    check(C > 0 && H >= 4 + C * kw + 1 && H % 4 == 0, "bad exchange row geometry");
    check(send.numel() == G * H, "send must be [G * H]");
    psamd::xchg_pack_keys(ptr<uint64_t>(ukeys), ptr<int32_t>(n_uniq), ukeys.numel(),
                          ptr<int64_t>(off), G, C, kw, H, ptr<int32_t>(send),
                          optr<int32_t>(ovf, at::kInt, "ovf"), cur_stream());
  }, py::arg("ukeys"), py::arg("n_uniq"), py::arg("off"), py::arg("C"), py::arg("kw"),
     py::arg("H"), py::arg("send"), py::arg("ovf"));
  m.def("xchg_pack_grads", [](Tensor grad, optional<Tensor> perm, Tensor n_uniq, Tensor off,
                              int64_t C, int kw, int64_t H, Tensor send, optional<Tensor> hist,
                              optional<Tensor> metrics, optional<Tensor> step_counter,
                              optional<Tensor> ovf, optional<Tensor> ovf_host) {
    chk(grad, at::kFloat, "grad");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(off, at::kLong, "off");
    chk(send, at::kInt, "send");
    const int G = (int)off.numel() - 1;
    check(G >= 1 && G <= 64, "1..64 peers");
    check(C > 0 && H >= 4 + C * (kw + 1) && H % 4 == 0, "bad exchange row geometry");
    check(send.numel() == G * H, "send must be [G * H]");
    const int32_t* pp = optr<int32_t>(perm, at::kInt, "perm");
    if (pp) check(perm->numel() >= grad.numel(), "perm shorter than grad");
    // optional: the step's AUC histogram (stripes x 2 x 2048) -> metrics in block 0
    psamd::AucOut auc = auc_out(
        hist, metrics, "xchg_pack_grads: hist = stripes x 2 x 2048 (<= 8 stripes) with metrics");
    auc.step_counter = step_counter_of(step_counter);
    psamd::xchg_pack_grads(ptr<float>(grad), pp, ptr<int32_t>(n_uniq), grad.numel(),
                           ptr<int64_t>(off), G, C, kw, H, ptr<int32_t>(send), auc,
                           optr<int32_t>(ovf, at::kInt, "ovf"), host_flag(ovf, ovf_host),
                           cur_stream());
  }, py::arg("grad"), py::arg("perm"), py::arg("n_uniq"), py::arg("off"), py::arg("C"),
     py::arg("kw"), py::arg("H"), py::arg("send"), py::arg("hist") = py::none(),
     py::arg("metrics") = py::none(), py::arg("step_counter") = py::none(),
     py::arg("ovf") = py::none(), py::arg("ovf_host") = py::none());
  m.def("xchg_ff_pack_grads", [](Tensor grad, optional<Tensor> perm, Tensor n_uniq, Tensor off,
                                 int64_t C, int kw, int64_t H, int nb, uint64_t seed,
                                 optional<Tensor> step, Tensor send, Tensor gstage) {
    chk(grad, at::kFloat, "grad");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(off, at::kLong, "off");
    chk(send, at::kInt, "send");
    chk(gstage, at::kFloat, "gstage");
    const int G = (int)off.numel() - 1;
    check(G >= 1 && G <= 64, "1..64 peers");
    check(kw == 1 || kw == 2, "kw must be 1 or 2");
    check(nb >= 1 && nb <= 7, "FixingFloat bytes in [1, 7]");
    check(C > 0 && H >= 4 + C * kw + (C * nb + 3) / 4 && H % 4 == 0, "bad exchange row geometry");
    check(send.numel() == G * H, "send must be [G * H]");
    check(gstage.numel() >= G * C, "gstage < G*C");
    const int32_t* pp = optr<int32_t>(perm, at::kInt, "perm");
    if (pp) check(perm->numel() >= grad.numel(), "perm shorter than grad");
    psamd::xchg_ff_pack_grads(ptr<float>(grad), pp, ptr<int32_t>(n_uniq), grad.numel(),
                              ptr<int64_t>(off), G, C, kw, H, nb, seed,
                              optr<int64_t>(step, at::kLong, "step"), ptr<int32_t>(send),
                              ptr<float>(gstage), cur_stream());
  });
  m.def("xchg_ff_encode", [](Tensor gstage, int64_t C, int kw, int64_t H, int nb, uint64_t seed,
                             optional<Tensor> step, Tensor send, int per) {
    chk(gstage, at::kFloat, "gstage");
    chk(send, at::kInt, "send");
    check(kw == 1 || kw == 2, "kw must be 1 or 2");
    check(nb >= 1 && nb <= 7, "FixingFloat bytes in [1, 7]");
    check(C > 0 && H >= 4 + C * kw + (C * nb + 3) / 4 && send.numel() % H == 0,
          "bad exchange row geometry");
    const int G = (int)(send.numel() / H);
    check(G >= 1 && G <= 64 && gstage.numel() >= G * C, "gstage < G*C");
    check(per >= 0 && gstage.numel() >= G * C + 2 * (int64_t)G * per,
          "xchg_ff_encode: gstage < G*C + the producers' partials");
    psamd::xchg_ff_encode(ptr<float>(gstage), G, C, kw, H, nb, seed,
                          optr<int64_t>(step, at::kLong, "step"), ptr<int32_t>(send), per,
                          cur_stream());
  }, py::arg("gstage"), py::arg("C"), py::arg("kw"), py::arg("H"), py::arg("nb"), py::arg("seed"),
     py::arg("step"), py::arg("send"), py::arg("per") = 0);
  m.def("xchg_ff_decode", [](Tensor recv, int64_t C, int kw, int64_t H, int nb, Tensor gin) {
    chk(recv, at::kInt, "recv");
    chk(gin, at::kFloat, "gin");
    check(kw == 1 || kw == 2, "kw must be 1 or 2");
    check(nb >= 1 && nb <= 7, "FixingFloat bytes in [1, 7]");
    check(C > 0 && H >= 4 + C * kw + (C * nb + 3) / 4 && H % 4 == 0, "bad exchange row geometry");
    const int G = exchange_rows(recv, H, C, 4, "recv is not a whole number of rows");
    check(gin.numel() >= G * C, "gin < G*C");
    psamd::xchg_ff_decode(ptr<int32_t>(recv), G, C, kw, H, nb, ptr<float>(gin), cur_stream());
  });
  m.def("xchg_clear_counts", [](Tensor send, int64_t H, bool keys, bool grads) {
    chk(send, at::kInt, "send");
    const int G = exchange_rows(send, H, 1, 5, "send is not a whole number of rows");
    psamd::xchg_clear_counts(ptr<int32_t>(send), G, H, keys, grads, cur_stream());
  });
  m.def("xchg_unpack_w", [](Tensor recv_w, optional<Tensor> perm, Tensor n_uniq, Tensor off,
                            int64_t C, Tensor w_local, int64_t wstride) {
    const int64_t ws = wstride > 0 ? wstride : C;
    chk(recv_w, at::kFloat, "recv_w");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(off, at::kLong, "off");
    chk(w_local, at::kFloat, "w_local");
    const int G = (int)off.numel() - 1;
    check(G >= 1 && G <= 64, "1..64 peers");
    check(ws >= C && recv_w.numel() >= (G - 1) * ws + C, "recv_w < (G-1)*wstride + C");
    const int32_t* pp = optr<int32_t>(perm, at::kInt, "perm");
    if (pp) check(perm->numel() >= w_local.numel(), "perm shorter than w_local");
    psamd::xchg_unpack_w(ptr<float>(recv_w), pp, ptr<int32_t>(n_uniq), w_local.numel(),
                         ptr<int64_t>(off), G, C, ws, ptr<float>(w_local), cur_stream());
  }, py::arg("recv_w"), py::arg("perm"), py::arg("n_uniq"), py::arg("off"), py::arg("C"),
     py::arg("w_local"), py::arg("wstride") = 0);

  // ---------------- k-value push / pull API (kvapi.hip) ----------------
  // rows [hdr 4 | keys C*kw | values C*k f32] of H words (pull rows: no values)
  m.def("kvv_pack_vals", [](Tensor vals, int64_t k, Tensor pos_s, Tensor seg_start, Tensor n_uniq,
                            Tensor off, int64_t C, int kw, int64_t H, Tensor send) {
    chk(vals, at::kFloat, "vals");
    chk(pos_s, at::kInt, "pos_s");
    chk(seg_start, at::kInt, "seg_start");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(off, at::kLong, "off");
    chk(send, at::kInt, "send");
    const int G = (int)off.numel() - 1;
    check(G >= 1 && G <= 64, "1..64 peers");
    check(k >= 1 && vals.numel() % k == 0, "vals must be [nnz, k]");
    const int64_t nnz = vals.numel() / k;
    check(pos_s.numel() >= nnz, "pos_s < nnz");
    const int64_t u_cap = std::min<int64_t>(seg_start.numel() - 1, nnz);
    check(u_cap >= 1, "seg_start too small");
    check(kw >= 0 && kw <= 2, "kw must be 0 (key-less row of a registered key set), 1 or 2");
    check(C > 0 && H >= 4 + C * kw + C * k && H % 4 == 0, "bad push row geometry");
    check(send.numel() == G * H, "send must be [G * H]");
    psamd::kvv_pack_vals(ptr<float>(vals), (int)k, ptr<int32_t>(pos_s), ptr<int32_t>(seg_start),
                         ptr<int32_t>(n_uniq), u_cap, nnz, ptr<int64_t>(off), G, C, kw, H,
                         ptr<int32_t>(send), cur_stream());
  });
  m.def("kvv_serve", [](Tensor recv, int64_t H, int64_t C, Tensor slot, Tensor vals, Tensor rec) {
    chk(recv, at::kInt, "recv");
    chk(slot, at::kLong, "slot");
    chk(vals, at::kFloat, "vals");
    chk(rec, at::kFloat, "rec");
    const int G = exchange_rows(recv, H, C, 4);
    check(vals.dim() == 2, "vals must be [capacity, k]");
    const int64_t k = vals.size(1);
    check(slot.numel() >= G * C && rec.numel() >= G * C * k, "slot / rec < G*C(*k)");
    psamd::kvv_serve(ptr<int32_t>(recv), G, H, C, ptr<int64_t>(slot), ptr<float>(vals),
                     vals.size(0), (int)k, k, ptr<float>(rec), cur_stream());
  });
  // scalar tables (optimizer rules): serve the w field of the 32-B KV slots
  m.def("kv_serve_w", [](Tensor recv, int64_t H, int64_t C, Tensor slot, Tensor slots, Tensor rec) {
    chk(recv, at::kInt, "recv");
    chk(slot, at::kLong, "slot");
    chk(rec, at::kFloat, "rec");
    const int64_t cap = slot_capacity(slots);
    const int G = exchange_rows(recv, H, C, 4);
    check(slot.numel() >= G * C && rec.numel() >= G * C, "slot / rec < G*C");
    const float* w = reinterpret_cast<const float*>(static_cast<const char*>(slots.data_ptr()) + 8);
    psamd::kvv_serve(ptr<int32_t>(recv), G, H, C, ptr<int64_t>(slot), w, cap, 1, 8,
                     ptr<float>(rec), cur_stream());
  });
  m.def("kvv_apply", [](Tensor recv, int64_t H, int64_t C, int kw, Tensor slot, Tensor vals,
                        int op) {
    chk(recv, at::kInt, "recv");
    chk(slot, at::kLong, "slot");
    chk(vals, at::kFloat, "vals");
    check(op == 0 || op == 1, "op: 0 = add, 1 = assign");
    check(vals.dim() == 2, "vals must be [capacity, k]");
    const int64_t k = vals.size(1);
    check(kw >= 0 && kw <= 2, "kw must be 0 (key-less row), 1 or 2");
    const int G = exchange_rows(recv, H, C, 4 + C * kw + C * k, "bad push row geometry");
    check(slot.numel() >= G * C, "slot < G*C");
    psamd::kvv_apply(ptr<int32_t>(recv), G, H, C, kw, ptr<int64_t>(slot), ptr<float>(vals),
                     vals.size(0), (int)k, op, cur_stream());
  });
  m.def("kvv_unpack", [](Tensor rec, int64_t C, int64_t k, Tensor off, Tensor local_col,
                         Tensor out) {
    chk(rec, at::kFloat, "rec");
    chk(off, at::kLong, "off");
    chk(local_col, at::kInt, "local_col");
    chk(out, at::kFloat, "out");
    const int G = (int)off.numel() - 1;
    check(G >= 1 && G <= 64, "1..64 peers");
    check(k >= 1 && C > 0 && rec.numel() >= G * C * k, "rec < G*C*k");
    const int64_t nnz = local_col.numel();
    check(out.numel() >= nnz * k, "out < nnz*k");
    psamd::kvv_unpack(ptr<float>(rec), C, (int)k, ptr<int64_t>(off), G, ptr<int32_t>(local_col),
                      nnz, ptr<float>(out), cur_stream());
  });
  m.def("kvv_single_off", [](Tensor n_uniq, Tensor off) {
    chk(n_uniq, at::kInt, "n_uniq");
    chk(off, at::kLong, "off");
    check(off.numel() == 2, "off must be [2]");
    psamd::kvv_single_off(ptr<int32_t>(n_uniq), ptr<int64_t>(off), cur_stream());
  });

  // ---------------- one-sided peer-HBM exchange (p2p.hip) ----------------
  m.def("ipc_export", [](Tensor t) {
    check(t.is_cuda(), "ipc_export: device tensor");
    std::string out(72, '\0');
    psamd::ipc_export(t.data_ptr(), reinterpret_cast<uint8_t*>(&out[0]));
    return py::bytes(out);
  });
  m.def("ipc_import", [](py::bytes b) {
    std::string s = b;
    check(s.size() == 72, "ipc_import: 72-byte handle");
    return (int64_t) reinterpret_cast<intptr_t>(psamd::ipc_import(reinterpret_cast<const uint8_t*>(s.data())));
  });
  m.def("ipc_close", [](int64_t ptr, int64_t off) {
    psamd::ipc_close(reinterpret_cast<void*>(static_cast<intptr_t>(ptr)), off);
  });
  m.def("p2p_lookup_rows", [](Tensor tabs, int G, int self, Tensor send, int64_t H, int64_t C, int kw,
                              Tensor wout, Tensor slot_out, int init_type, double init_v,
                              double init_s, uint64_t seed, Tensor err,
                              optional<Tensor> inserted) {
    chk(tabs, at::kLong, "tabs");
    chk(send, at::kInt, "send");
    chk(wout, at::kFloat, "wout");
    chk(slot_out, at::kLong, "slot_out");
    chk(err, at::kInt, "err");
    check(G >= 1 && G <= 64 && self >= 0 && self < G, "p2p: 1..64 ranks");
    check(tabs.numel() == 5 * G, "tabs: 5 int64 per rank");
    check(kw == 1 || kw == 2, "kw 1 or 2");
    check(H >= 4 + C * kw, "row too short (header + C keys)");
    check(send.numel() >= G * H && wout.numel() >= G * C && slot_out.numel() >= G * C,
          "p2p_lookup_rows buffers too small");
    psamd::p2p_lookup_rows(tabs.data_ptr(), G, self, ptr<int32_t>(send), H, C, kw, ptr<float>(wout),
                           ptr<int64_t>(slot_out), key_init(init_type, init_v, init_s, seed),
                           ptr<int32_t>(err), optr<int32_t>(inserted, at::kInt, "inserted"),
                           cur_stream());
  });
  // rings: per peer the base of its inbox = G x Q entries of H words + G x Q sequence words
  m.def("p2p_post", [](Tensor send, int64_t H, int64_t C, int kw, int nb, int G, int self,
                       int64_t seq, int Q, Tensor rings, Tensor applied, Tensor ok, Tensor err,
                       optional<Tensor> err_host, int64_t spin) {
    chk(send, at::kInt, "send");
    chk(rings, at::kLong, "rings");
    chk(applied, at::kLong, "applied");
    chk(ok, at::kInt, "ok");
    chk(err, at::kInt, "err");
    check(G >= 1 && G <= 64 && self >= 0 && self < G, "p2p: 1..64 ranks");
    check(nb >= 0 && nb <= 7, "p2p_post: FixingFloat 0..7 bytes");
    check(rings.numel() == G && applied.numel() == G && ok.numel() >= G, "p2p_post: G pointers");
    const int64_t gw = nb ? (C * nb + 3) / 4 : C;
    check(send.numel() >= G * H && H >= 4 + C * kw + gw, "p2p_post: send rows");
    check(seq >= 1 && seq < (int64_t(1) << 31) && Q >= 1, "p2p_post: 1 <= seq < 2^31, Q >= 1");
    int32_t* eh = nullptr;
    if (err_host.has_value() && err_host->defined())
      eh = pinned_word(*err_host, "err_host must be a pinned int32 host tensor");
    psamd::p2p_post(ptr<int32_t>(send), H, C, kw, nb, G, self, (int32_t)seq, Q,
                    reinterpret_cast<void* const*>(rings.data_ptr()),
                    reinterpret_cast<void* const*>(applied.data_ptr()), ptr<int32_t>(ok),
                    ptr<int32_t>(err), eh, spin, cur_stream());
  });
  m.def("p2p_gather", [](Tensor inbox, Tensor applied, int G, int self, int Q, int64_t H, int64_t C,
                         int kw, int nb, Tensor stage, Tensor ready) {
    chk(inbox, at::kInt, "inbox");
    chk(applied, at::kInt, "applied");
    chk(stage, at::kInt, "stage");
    chk(ready, at::kInt, "ready");
    check(G >= 1 && G <= 64 && self >= 0 && self < G, "p2p: 1..64 ranks");
    check(nb >= 0 && nb <= 7, "p2p_gather: FixingFloat 0..7 bytes");
    check(inbox.numel() >= (int64_t)G * Q * (H + 1) && stage.numel() >= G * H,
          "p2p_gather: inbox = G x Q x (H + 1) words");
    check(applied.numel() >= G && ready.numel() >= G, "p2p_gather: counters");
    psamd::p2p_gather(ptr<int32_t>(inbox), ptr<int32_t>(applied), G, self, Q, H, C, kw, nb,
                      ptr<int32_t>(stage), ptr<int32_t>(ready), cur_stream());
  });
  // a zeroed FINE-GRAINED device buffer (cross-device coherent while kernels run; IPC
  // exportable) as a uint8 tensor that frees itself
  m.def("fine_empty", [](int64_t nbytes) {
    check(nbytes > 0, "fine_empty: nbytes > 0");
    int dev = 0;
    PSAMD_HIP_CHECK(hipGetDevice(&dev));
    void* p = psamd::p2p_fine_alloc((size_t)nbytes);
    return torch::from_blob(p, {nbytes}, [](void* q) { psamd::p2p_fine_free(q); },
                            torch::TensorOptions().dtype(at::kByte).device(at::kCUDA, dev));
  });
  m.def("p2p_commit", [](Tensor applied, Tensor ready, int G, optional<Tensor> total) {
    chk(applied, at::kInt, "applied");
    chk(ready, at::kInt, "ready");
    check(G >= 1 && G <= 64 && applied.numel() >= G && ready.numel() >= G, "p2p_commit");
    psamd::p2p_commit(ptr<int32_t>(applied), ptr<int32_t>(ready), G,
                      optr<int64_t>(total, at::kLong, "total"), cur_stream());
  });
}
