// Shared by the binding units (bind*.cpp): argument checks, the validators several ops
// share, the launch list and the registration hooks. Every op validates device / dtype /
// contiguity and sizes on the host BEFORE launching, so a malformed call raises instead
// of faulting the GPU.
#pragma once
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "common.cuh"
#include "kv_slot.cuh"
#include "params.h"

namespace psamd_bind {

using at::Tensor;
using c10::optional;
namespace py = pybind11;

// One hook per binding unit; PYBIND11_MODULE (bind.cpp) calls them in this order
// (register_launch first: the others add methods to its LaunchList).
void register_launch(py::module_& m);    // LaunchList, GraphChain, events
void register_table(py::module_& m);     // KV table, exchange rows, k-value API, p2p
void register_tploc(py::module_& m);     // tile / flat localiser, fused step
void register_prep(py::module_& m);      // localisation, sort / scan / RLE, filters, text
void register_linear(py::module_& m);    // linear / predict / FM, the generator
void register_dense(py::module_& m);     // Darlin BCD, GEMMs, embedding, spmv
void register_scoretext(py::module_& m); // prediction lines
void register_slotsplit(py::module_& m); // split by feature group

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void check(bool ok, const std::string& msg) {
  if (!ok) throw std::invalid_argument(msg);
}

inline void chk(const Tensor& t, at::ScalarType dt, const char* name) {
  check(t.is_cuda(), std::string(name) + ": must be a GPU tensor");
  check(t.is_contiguous(), std::string(name) + ": must be contiguous");
  check(t.scalar_type() == dt, std::string(name) + ": wrong dtype " +
                                   std::string(c10::toString(t.scalar_type())));
}

template <typename T>
T* ptr(const Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }

template <typename T>
T* optr(const optional<Tensor>& t, at::ScalarType dt, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  chk(*t, dt, name);
  return reinterpret_cast<T*>(t->data_ptr());
}

inline uint64_t inv_mod64(uint64_t a) {  // a odd; Newton iteration for a^-1 mod 2^64
  uint64_t x = a;
  for (int i = 0; i < 6; ++i) x *= 2 - a * x;
  return x;
}

inline psamd::KeyMix make_keymix(int bits) {
  check(bits >= 2 && bits <= 64, "key bits must be in [2, 64]");
  psamd::KeyMix m;
  m.bits = bits;
  m.mask = bits == 64 ? ~0ull : ((1ull << bits) - 1);
  m.a = 0xbf58476d1ce4e5b9ull & m.mask;
  m.b = 0x94d049bb133111ebull & m.mask;
  m.a |= 1;
  m.b |= 1;
  m.ai = inv_mod64(m.a) & m.mask;
  m.bi = inv_mod64(m.b) & m.mask;
  m.s = (bits + 1) / 2;
  return m;
}

// Stripe count of a contended-accumulator buffer (common.cuh acc_stripe).
inline int acc_stripes_of(const Tensor& t) {
  return t.numel() >= psamd::kAccStripes * psamd::kAccStride ? psamd::kAccStripes : 1;
}
inline int acc_stripes_of(const optional<Tensor>& t) {
  return t.has_value() && t->defined() ? acc_stripes_of(*t) : 1;
}

inline int64_t slot_capacity(const Tensor& slots) {
  chk(slots, at::kLong, "slots");
  check(slots.dim() == 2 && slots.size(1) == 4, "slots must be [capacity, 4] int64 (32-B slots)");
  const int64_t cap = slots.size(0);
  check(cap > 0 && (cap & (cap - 1)) == 0, "slot capacity must be a power of two");
  return cap;
}

// ---- parsers of the argument groups (params.h)
inline psamd::TableRef table_ref(const Tensor& slots, uint64_t home_base, uint64_t home_m) {
  return {slots.data_ptr(), slot_capacity(slots), home_base, home_m};
}

inline psamd::KeyInit key_init(int init_type, double init_v, double init_s, uint64_t seed) {
  return {init_type, (float)init_v, (float)init_s, seed};
}

inline psamd::UpdateParams update_params(int algo, int lr_type, double alpha, double beta,
                                         double l1, double l2, double grad_scale,
                                         double max_delta) {
  return {algo, lr_type, (float)alpha, (float)beta, (float)l1, (float)l2, (float)grad_scale,
          (float)max_delta};
}

// an optional striped f64 accumulator (stats / metrics)
inline psamd::StripedAcc striped_acc(const optional<Tensor>& t, const char* name) {
  return {optr<double>(t, at::kDouble, name), acc_stripes_of(t)};
}

// The AUC a step folds into one of its launches: hist = stripes x 2 x 2048 int32 with
// metrics. `bad_hist`: the op's message for a malformed hist. step_counter stays null:
// the op parses it (step_counter_of) where its argument order has it.
inline psamd::AucOut auc_out(const optional<Tensor>& hist, const optional<Tensor>& metrics,
                             const std::string& bad_hist) {
  constexpr int kBins = 2048;
  uint32_t* hp = optr<uint32_t>(hist, at::kInt, "hist");
  double* mp = optr<double>(metrics, at::kDouble, "metrics");
  if (hp) check(mp && hist->numel() % (2 * kBins) == 0 && hist->numel() / (2 * kBins) <= 8,
                bad_hist);
  return {hp, kBins, hp ? (int)(hist->numel() / (2 * kBins)) : 1, mp, nullptr};
}
inline int64_t* step_counter_of(const optional<Tensor>& step_counter) {
  return optr<int64_t>(step_counter, at::kLong, "step_counter");
}

// ---- exchange rows (exchange.hip): rows = G rows of H int32 words with up to C keys
// each; min_h: the least H the op's row layout needs. Returns G (1..64 peers).
inline int exchange_rows(const Tensor& rows, int64_t H, int64_t C, int64_t min_h,
                         const char* bad = "bad exchange row geometry") {
  check(C > 0 && H >= min_h && rows.numel() % H == 0, bad);
  const int G = (int)(rows.numel() / H);
  check(G >= 1 && G <= 64, "1..64 peers");
  return G;
}
// gradient row s at grad[s * gstride]
inline void check_grad_rows(const Tensor& grad, int64_t gstride, int G, int64_t C) {
  check(gstride >= C && grad.numel() >= (G - 1) * gstride + C, "grad rows out of bounds");
}

// device-visible pointer of a pinned int32 host word (`what`: the message when it is not)
inline int32_t* pinned_word(const Tensor& host, const char* what) {
  check(host.device().is_cpu() && host.is_pinned() && host.scalar_type() == at::kInt &&
            host.numel() >= 1, what);
  void* dptr = nullptr;
  PSAMD_HIP_CHECK(hipHostGetDevicePointer(&dptr, host.data_ptr(), 0));
  return reinterpret_cast<int32_t*>(dptr);
}

// ---- validate-once launchers (the single ops and LaunchList share them) ----
using Launch = std::function<void(hipStream_t)>;
// A launch list op gets the list's current stream by reference: kernel ops launch on
// it, control ops switch it or order it against events (a multi-stream iteration of the
// data pipeline as ONE host call, bench.py).
using Op = std::function<void(hipStream_t&)>;
struct LaunchList {
  std::vector<Op> ops;
  std::vector<const char*> names;  // per op (a failing op is named in the error)
  std::vector<py::object> keep;    // the torch streams / events the control ops use
  void push(Launch l, const char* name) {
    ops.push_back([l](hipStream_t& s) { l(s); });
    names.push_back(name);
  }
  void push_op(Op o, const char* name) {
    ops.push_back(std::move(o));
    names.push_back(name);
  }
};

inline py::class_<LaunchList> launch_list_class(py::module_& m) {
  return py::reinterpret_borrow<py::class_<LaunchList>>(m.attr("LaunchList"));
}

// An op whose parameter list is written once, as its make_* function (validate, then
// return the launch): def_eager registers m.<name>(args...), which launches on the
// current stream; def_launch also registers LaunchList.add_<name>(args...), which
// appends the launch. `extra`: the eager op's py::args (add_* stay positional).
template <typename... A, typename... Extra>
void def_eager(py::module_& m, const char* name, Launch (*make)(A...), const Extra&... extra) {
  m.def(name, [make](A... a) { make(std::move(a)...)(cur_stream()); }, extra...);
}
template <typename... A, typename... Extra>
void def_launch(py::module_& m, const char* name, Launch (*make)(A...), const Extra&... extra) {
  def_eager(m, name, make, extra...);
  launch_list_class(m).def((std::string("add_") + name).c_str(), [make, name](LaunchList& l, A... a) {
    l.push(make(std::move(a)...), name);
  });
}

}  // namespace psamd_bind
