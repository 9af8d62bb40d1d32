// Python bindings of _hipops (torch tensors in, kernels on the current HIP stream): the
// module, which only calls the binding units' registration hooks (bind_common.h), and the
// dense unit -- Darlin BCD (bcd.hip), the bf16 GEMMs (gemm.hip, gemm256.hip), embeddings /
// wide & deep / Adam (embedding.hip) and spmv (spmv.hip). The other kernel families are
// bound in bind_launch.cpp, bind_table.cpp, bind_tploc.cpp, bind_prep.cpp, bind_linear.cpp,
// bind_scoretext.cpp, bind_slotsplit.cpp.
#include <cmath>

#include "bcd.h"
#include "bind_common.h"
#include "embedding.h"
#include "gemm.h"
#include "gemm256.h"
#include "spmv.h"

using namespace psamd_bind;

void psamd_bind::register_dense(py::module_& m) {
  // ---------------- 256x256 LDS-DMA bf16 GEMM, K-major operands (gemm256.hip) ----------------
  m.def("gemm_nt256", [](Tensor A, Tensor B, int64_t M, int64_t N, int64_t K,
                         optional<Tensor> bias, bool relu, optional<Tensor> C,
                         optional<Tensor> Cf, int variant) {
    chk(A, at::kBFloat16, "A");
    chk(B, at::kBFloat16, "B");
    check(M > 0 && N > 0 && K > 0 && K % 64 == 0, "gemm_nt256: K must be a multiple of 64");
    check(A.numel() >= M * K && B.numel() >= N * K, "gemm_nt256: A [M, K], B [N, K]");
    check(((uintptr_t)A.data_ptr() % 16) == 0 && ((uintptr_t)B.data_ptr() % 16) == 0,
          "gemm_nt256: 16-B aligned operands");
    const float* bp = optr<float>(bias, at::kFloat, "bias");
    if (bp) check(bias->numel() >= N, "bias too small");
    __bf16* cp = C.has_value() && C->defined() ? (chk(*C, at::kBFloat16, "C"), ptr<__bf16>(*C)) : nullptr;
    float* fp = optr<float>(Cf, at::kFloat, "Cf");
    check(cp || fp, "gemm_nt256: need an output");
    if (cp) check(C->numel() >= M * N, "C too small");
    if (fp) check(Cf->numel() >= M * N, "Cf too small");
    check(variant >= 0 && variant <= 6,
          "variant: 0 = one barrier per K-step, 1 = ping-pong, 2 = ping-pong with 2-step "
          "prefetch, 3 = 0 with fragment reads interleaved into the MFMA rows, 4 = 4-slot "
          "LDS ring, 5 = 4 waves of 128 x 128, 6 = 4 with 32x32x16 MFMAs");
    psamd::gemm_nt256(ptr<__bf16>(A), K, ptr<__bf16>(B), K, (int)M, (int)N, (int)K, bp, relu, cp, N,
                      fp, N, variant, cur_stream());
  }, py::arg("A"), py::arg("B"), py::arg("M"), py::arg("N"), py::arg("K"), py::arg("bias"),
     py::arg("relu"), py::arg("C"), py::arg("Cf"), py::arg("variant") = 0);
  // C [M, N] f32 = beta C + A^T B for MN-major A [K, M], B [K, N] (the weight gradient):
  // split-K partials into part [splits, M, N], then a fixed-order sum (gemm256.hip)
  m.def("gemm_tn256", [](Tensor A, Tensor B, int64_t M, int64_t N, int64_t K, int64_t splits,
                         Tensor part, Tensor C, double beta, int phase,
                         optional<Tensor> tile_ctr) {
    chk(A, at::kBFloat16, "A");
    chk(B, at::kBFloat16, "B");
    chk(part, at::kFloat, "part");
    chk(C, at::kFloat, "C");
    check(M > 0 && N > 0 && K > 0 && K % 64 == 0 && M % 8 == 0 && N % 8 == 0,
          "gemm_tn256: K % 64, M % 8, N % 8");
    check(splits >= 1 && splits <= K / 64, "gemm_tn256: 1 <= splits <= K / 64");
    check(A.numel() >= K * M && B.numel() >= K * N, "gemm_tn256: A [K, M], B [K, N]");
    check(part.numel() >= splits * M * N && C.numel() >= M * N, "gemm_tn256: part / C size");
    check(((uintptr_t)A.data_ptr() % 16) == 0 && ((uintptr_t)B.data_ptr() % 16) == 0 &&
              ((uintptr_t)C.data_ptr() % 16) == 0 && ((uintptr_t)part.data_ptr() % 16) == 0,
          "gemm_tn256: 16-B aligned operands");
    check(phase >= 0 && phase <= 3,
          "gemm_tn256: phase 0 (both) / 1 (GEMM) / 2 (reduce) / 3 (reduce in the GEMM)");
    auto* tc = reinterpret_cast<unsigned int*>(optr<int32_t>(tile_ctr, at::kInt, "tile_ctr"));
    if (phase == 3)
      check(tc && tile_ctr->numel() >= ((M + 255) / 256) * ((N + 255) / 256),
            "gemm_tn256 phase 3: tile_ctr, one zeroed int32 per 256 x 256 tile");
    psamd::gemm_tn256(ptr<__bf16>(A), M, ptr<__bf16>(B), N, (int)M, (int)N, (int)K, (int)splits,
                      ptr<float>(part), ptr<float>(C), (float)beta, phase, tc, cur_stream());
  }, py::arg("A"), py::arg("B"), py::arg("M"), py::arg("N"), py::arg("K"), py::arg("splits"),
     py::arg("part"), py::arg("C"), py::arg("beta"), py::arg("phase") = 0,
     py::arg("tile_ctr") = py::none());
  m.def("transpose_bf16", [](Tensor in, Tensor out) {
    chk(in, at::kBFloat16, "in");
    chk(out, at::kBFloat16, "out");
    check(in.dim() == 2 && out.numel() >= in.numel(), "transpose_bf16: in [R, C], out [C, R]");
    const int64_t R = in.size(0), C = in.size(1);
    check(R % 64 == 0 && C % 64 == 0, "transpose_bf16: R, C multiples of 64");
    psamd::transpose_bf16(in.data_ptr(), (int)R, (int)C, out.data_ptr(), cur_stream());
  });

  // ---------------------------------------------------------------- Darlin BCD
  // CSC of one rank: col/row int32 per nnz (sorted by col), val f32 per nnz or None
  // (binary). Block = nnz range [p0, p1) holding global columns [c0, c0 + ncols).
  auto csc_check = [](const Tensor& col, const Tensor& row, const optional<Tensor>& val,
                      int64_t p0, int64_t p1) {
    chk(col, at::kInt, "col");
    chk(row, at::kInt, "row");
    check(col.numel() == row.numel(), "col/row size mismatch");
    check(0 <= p0 && p0 <= p1 && p1 <= col.numel(), "nnz range outside the matrix");
    if (val.has_value() && val->defined()) {
      chk(*val, at::kFloat, "val");
      check(val->numel() == col.numel(), "val size mismatch");
    }
  };
  m.def("bcd_grad_chunked", [](Tensor col, Tensor row, optional<Tensor> val, Tensor chunks,
                                int64_t c0, int64_t ncols, Tensor ym, Tensor y, Tensor delta,
                                Tensor active, Tensor G, Tensor U, bool zeroed,
                                optional<Tensor> rowq, bool rowq_ready,
                                optional<Tensor> urows) {
    // chunks: [n + 1] int64 entry offsets (bit 62 = hot chunk), built and range-checked
    // on the host once per block (models/darlin.py build_chunks)
    chk(col, at::kInt, "col");
    chk(row, at::kInt, "row");
    chk(chunks, at::kLong, "chunks");
    check(chunks.numel() >= 1, "chunks needs the end sentinel");
    chk(ym, at::kDouble, "ym");
    chk(y, at::kFloat, "y");
    chk(delta, at::kDouble, "delta");
    chk(active, at::kByte, "active");
    chk(G, at::kDouble, "G");
    chk(U, at::kDouble, "U");
    check(row.numel() == col.numel(), "col/row size mismatch");
    const float* vp = optr<float>(val, at::kFloat, "val");
    if (vp) check(val->numel() == col.numel(), "val size mismatch");
    check(y.numel() == ym.numel(), "y/ym size mismatch");
    check(delta.numel() == active.numel(), "delta/active size mismatch");
    check(c0 >= 0 && ncols >= 0 && c0 + ncols <= delta.numel(), "column block outside model");
    check(G.numel() >= ncols && U.numel() >= ncols, "G/U too small");
    double* rq = optr<double>(rowq, at::kDouble, "rowq");
    if (rq) check(rowq->numel() >= 2 * ym.numel(), "rowq: 2 doubles per example");
    // urows: the block's distinct examples (the rowq packing covers only them; entries
    // outside the list would read stale factors: built from the block's rows, darlin.py)
    const int32_t* ur = optr<int32_t>(urows, at::kInt, "urows");
    if (ur) check(rq != nullptr, "urows needs rowq");
    psamd::bcd_grad_chunked(ptr<int32_t>(col), ptr<int32_t>(row), vp, ptr<int64_t>(chunks),
                            chunks.numel() - 1, c0, ncols, ptr<double>(ym), ptr<float>(y),
                            ym.numel(), ptr<double>(delta), ptr<uint8_t>(active), rq,
                            ptr<double>(G), ptr<double>(U), zeroed, rq != nullptr && rowq_ready,
                            ur, ur ? urows->numel() : 0, cur_stream());
  }, py::arg("col"), py::arg("row"), py::arg("val"), py::arg("chunks"), py::arg("c0"),
     py::arg("ncols"), py::arg("ym"), py::arg("y"), py::arg("delta"), py::arg("active"),
     py::arg("G"), py::arg("U"), py::arg("zeroed"), py::arg("rowq"), py::arg("rowq_ready"),
     py::arg("urows") = py::none());
  // Darlin row pass over dense per-row block layouts (bcd.hip bcd_rowpass): the pending
  // dual update of block j (jcol: [rows] int32 column relative to the block, -1 none)
  // fused with block k's gradient (narrow: part/G/U; wide: rowq).
  m.def("bcd_rowpass", [](Tensor ym, Tensor y, optional<Tensor> jcol, optional<Tensor> jval,
                          optional<Tensor> jdw, int64_t jncols, optional<Tensor> kcol,
                          optional<Tensor> kval, int64_t c0, int64_t ncols, Tensor delta,
                          Tensor active, int k2, int W, optional<Tensor> part,
                          optional<Tensor> G, optional<Tensor> U, optional<Tensor> rowq,
                          optional<Tensor> hcols, optional<Tensor> part2, bool tau32) {
    chk(ym, at::kDouble, "ym");
    chk(y, at::kFloat, "y");
    chk(delta, at::kDouble, "delta");
    chk(active, at::kByte, "active");
    const int64_t n = ym.numel();
    check(y.numel() == n, "y/ym size mismatch");
    const int32_t* jc = optr<int32_t>(jcol, at::kInt, "jcol");
    const float* jv = optr<float>(jval, at::kFloat, "jval");
    const double* jd = optr<double>(jdw, at::kDouble, "jdw");
    if (jc) {
      check(jcol->numel() == n, "jcol: one int32 per example");
      check(jd != nullptr && jncols >= 0 && jdw->numel() >= jncols, "jdw too small");
      if (jv) check(jval->numel() == n, "jval: one float per example");
    }
    const int32_t* kc = optr<int32_t>(kcol, at::kInt, "kcol");
    const float* kv = optr<float>(kval, at::kFloat, "kval");
    if (kc) {
      check(kcol->numel() == n, "kcol: one int32 per example");
      if (kv) check(kval->numel() == n, "kval: one float per example");
      check(c0 >= 0 && ncols >= 0 && c0 + ncols <= delta.numel(), "column block outside model");
    }
    long long* pp = optr<long long>(part, at::kLong, "part");
    double* Gp = optr<double>(G, at::kDouble, "G");
    double* Up = optr<double>(U, at::kDouble, "U");
    double* rq = optr<double>(rowq, at::kDouble, "rowq");
    const int32_t* hc = optr<int32_t>(hcols, at::kInt, "hcols");
    const int64_t nhot = hc ? hcols->numel() : 0;
    if (pp) {
      check(kc != nullptr, "LDS row pass needs kcol");
      const int64_t nl = hc ? nhot : ncols;
      check(nl <= psamd::bcd_rows_max_cols(), "bcd_rowpass: <= 2048 LDS columns");
      check(W >= 1 && part->numel() >= (int64_t)(W + psamd::bcd_part_segments()) * 2 * nl,
            "part: (W + bcd_part_segments) x 2 x LDS columns int64");
      check(Gp && Up && G->numel() >= ncols && U->numel() >= ncols, "G/U too small");
      check(k2 >= 0 && k2 <= 62, "fixed-point shift");
      // hot columns of a wide block (the reduce stores G[hcols[h]]): range-checked once
      // where they are built (ops/bcd.py hot_layout), not per call (no host sync here)
      if (hc) check(rq != nullptr && rowq->numel() >= 2 * n, "rowq: 2 doubles per example");
      if (part2.has_value() && part2->defined())
        check(part2->numel() >= (int64_t)psamd::bcd_part_segments() * 2 * nl,
              "part2: segments x 2 x LDS columns int64");
    } else if (kc) {
      check(rq != nullptr && rowq->numel() >= 2 * n, "rowq: 2 doubles per example");
    }
    psamd::bcd_rowpass(n, ptr<double>(ym), ptr<float>(y), jc, jv, jd, jncols, kc, kv, c0, ncols,
                       ptr<double>(delta), ptr<uint8_t>(active), k2, W, pp, Gp, Up, rq, hc, nhot,
                       optr<long long>(part2, at::kLong, "part2"), tau32, cur_stream());
  }, py::arg("ym"), py::arg("y"), py::arg("jcol"), py::arg("jval"), py::arg("jdw"),
     py::arg("jncols"), py::arg("kcol"), py::arg("kval"), py::arg("c0"), py::arg("ncols"),
     py::arg("delta"), py::arg("active"), py::arg("k2"), py::arg("W"), py::arg("part"),
     py::arg("G"), py::arg("U"), py::arg("rowq"), py::arg("hcols"), py::arg("part2"),
     py::arg("tau32") = false);
  m.def("bcd_grad", [csc_check](Tensor col, Tensor row, optional<Tensor> val, int64_t p0,
                                int64_t p1, int64_t c0, int64_t ncols, Tensor ym, Tensor y,
                                Tensor delta, Tensor active, Tensor G, Tensor U) {
    csc_check(col, row, val, p0, p1);
    chk(ym, at::kDouble, "ym");
    chk(y, at::kFloat, "y");
    chk(delta, at::kDouble, "delta");
    chk(active, at::kByte, "active");
    chk(G, at::kDouble, "G");
    chk(U, at::kDouble, "U");
    check(y.numel() == ym.numel(), "y/ym size mismatch");
    check(delta.numel() == active.numel(), "delta/active size mismatch");
    check(c0 >= 0 && ncols >= 0 && c0 + ncols <= delta.numel(), "column block outside model");
    check(G.numel() >= ncols && U.numel() >= ncols, "G/U too small");
    psamd::bcd_grad(ptr<int32_t>(col), ptr<int32_t>(row), optr<float>(val, at::kFloat, "val"), p0,
                    p1, c0, ncols, ptr<double>(ym), ptr<float>(y), ym.numel(), ptr<double>(delta),
                    ptr<uint8_t>(active), ptr<double>(G), ptr<double>(U), cur_stream());
  });
  m.def("bcd_update", [](int64_t c0, int64_t ncols, Tensor G, Tensor U, Tensor w, Tensor delta,
                         Tensor active, Tensor dw, double eta, double lambda, double delta_max,
                         double kkt_thr, Tensor vio_bits, bool consume, bool nan_filtered,
                         optional<Tensor> part2, int k2) {
    chk(G, at::kDouble, "G");
    chk(U, at::kDouble, "U");
    chk(w, at::kDouble, "w");
    chk(delta, at::kDouble, "delta");
    chk(active, at::kByte, "active");
    chk(dw, at::kDouble, "dw");
    chk(vio_bits, at::kLong, "vio_bits");
    check(w.numel() == delta.numel() && w.numel() == active.numel(), "model arrays mismatch");
    check(c0 >= 0 && ncols >= 0 && c0 + ncols <= w.numel(), "column block outside model");
    check(G.numel() >= ncols && U.numel() >= ncols && dw.numel() >= ncols, "G/U/dw too small");
    check(eta > 0, "eta must be > 0");
    const long long* p2 = optr<long long>(part2, at::kLong, "part2");
    if (p2)
      check(part2->numel() >= (int64_t)psamd::bcd_part_segments() * 2 * ncols && k2 >= 0 &&
                k2 <= 62,
            "part2: segments x 2 x ncols int64 (a narrow row pass's sums)");
    psamd::bcd_update(c0, ncols, ptr<double>(G), ptr<double>(U), ptr<double>(w),
                      ptr<double>(delta), ptr<uint8_t>(active), ptr<double>(dw), eta, lambda,
                      delta_max, kkt_thr, ptr<unsigned long long>(vio_bits), consume,
                      nan_filtered, p2, k2, cur_stream());
  });
  m.def("bcd_replica", [](int64_t c0, int64_t ncols, int64_t own0, int64_t own1, Tensor dw,
                          Tensor w, Tensor delta, Tensor active, double delta_max) {
    chk(dw, at::kDouble, "dw");
    chk(w, at::kDouble, "w");
    chk(delta, at::kDouble, "delta");
    chk(active, at::kByte, "active");
    check(w.numel() == delta.numel() && w.numel() == active.numel(), "model arrays mismatch");
    check(c0 >= 0 && ncols >= 0 && c0 + ncols <= w.numel(), "column block outside model");
    check(dw.numel() >= ncols, "dw too small");
    psamd::bcd_replica(c0, ncols, own0, own1, ptr<double>(dw), ptr<double>(w), ptr<double>(delta),
                       ptr<uint8_t>(active), delta_max, cur_stream());
  });
  m.def("bcd_dual", [csc_check](Tensor col, Tensor row, optional<Tensor> val, int64_t p0,
                                int64_t p1, int64_t c0, int64_t ncols, Tensor dw, Tensor y,
                                Tensor ym, bool unique_rows) {
    csc_check(col, row, val, p0, p1);
    chk(dw, at::kDouble, "dw");
    chk(y, at::kFloat, "y");
    chk(ym, at::kDouble, "ym");
    check(y.numel() == ym.numel(), "y/ym size mismatch");
    check(ncols >= 0 && dw.numel() >= ncols, "dw too small");
    psamd::bcd_dual(ptr<int32_t>(col), ptr<int32_t>(row), optr<float>(val, at::kFloat, "val"), p0,
                    p1, c0, ncols, ptr<double>(dw), ptr<float>(y), ptr<double>(ym), ym.numel(),
                    unique_rows, cur_stream());
  });
  m.def("bcd_rows_max_cols", []() { return psamd::bcd_rows_max_cols(); });
  m.def("bcd_part_segments", []() { return psamd::bcd_part_segments(); });
  m.def("bcd_grad_rows", [csc_check](Tensor col, Tensor row, optional<Tensor> val, int64_t p0,
                                     int64_t p1, int64_t c0, int64_t ncols, Tensor ym, Tensor y,
                                     Tensor delta, Tensor active, int k2, int W, Tensor part,
                                     Tensor G, Tensor U, optional<Tensor> w,
                                     optional<Tensor> dw, optional<Tensor> vio_bits,
                                     optional<Tensor> counter, double eta, double lambda,
                                     double delta_max, double kkt_thr) {
    csc_check(col, row, val, p0, p1);
    chk(ym, at::kDouble, "ym");
    chk(y, at::kFloat, "y");
    chk(delta, at::kDouble, "delta");
    chk(active, at::kByte, "active");
    chk(part, at::kLong, "part");
    chk(G, at::kDouble, "G");
    chk(U, at::kDouble, "U");
    check(y.numel() == ym.numel(), "y/ym size mismatch");
    check(ncols >= 0 && ncols <= psamd::bcd_rows_max_cols(), "bcd_grad_rows: ncols <= 2048");
    check(c0 >= 0 && c0 + ncols <= delta.numel() && delta.numel() == active.numel(),
          "block columns out of range");
    check(G.numel() >= ncols && U.numel() >= ncols, "G/U too small");
    check(W >= 1 && W <= 65535 &&
              part.numel() >= (int64_t)(dw.has_value() && dw->defined() ? 1 : W) * 2 * ncols,
          "partials buffer (fused update: the block's 2 x ncols accumulator)");
    check(k2 >= 0 && k2 <= 62, "fixed-point scale 2^0..2^62");
    // fused update (dw given): the last workgroup applies the coordinate step of every
    // column of the block (bcd_update's arithmetic) and writes dw
    double* dwp = optr<double>(dw, at::kDouble, "dw");
    double* wp = optr<double>(w, at::kDouble, "w");
    auto* vp = reinterpret_cast<unsigned long long*>(optr<int64_t>(vio_bits, at::kLong, "vio_bits"));
    auto* cp = reinterpret_cast<unsigned int*>(optr<int32_t>(counter, at::kInt, "counter"));
    if (dwp) {
      check(wp && vp && cp, "fused update needs w, vio_bits and counter");
      check(w->numel() == delta.numel() && dw->numel() >= ncols, "w / dw size");
      check(eta > 0, "eta must be > 0");
    }
    psamd::bcd_grad_rows(ptr<int32_t>(col), ptr<int32_t>(row), optr<float>(val, at::kFloat, "val"),
                         p0, p1, c0, ncols, ptr<double>(ym), ptr<float>(y), ym.numel(),
                         ptr<double>(delta), ptr<uint8_t>(active), k2, W,
                         reinterpret_cast<long long*>(part.data_ptr()), ptr<double>(G),
                         ptr<double>(U), wp, dwp, vp, cp, eta, lambda, delta_max, kkt_thr,
                         cur_stream());
  }, py::arg("col"), py::arg("row"), py::arg("val"), py::arg("p0"), py::arg("p1"), py::arg("c0"),
     py::arg("ncols"), py::arg("ym"), py::arg("y"), py::arg("delta"), py::arg("active"),
     py::arg("k2"), py::arg("W"), py::arg("part"), py::arg("G"), py::arg("U"),
     py::arg("w") = py::none(), py::arg("dw") = py::none(), py::arg("vio_bits") = py::none(),
     py::arg("counter") = py::none(), py::arg("eta") = 1.0, py::arg("lam") = 0.0,
     py::arg("delta_max") = 0.0, py::arg("kkt_thr") = 0.0);
  m.def("bcd_objective", [](Tensor ym, Tensor out) {
    chk(ym, at::kDouble, "ym");
    chk(out, at::kDouble, "out");
    check(out.numel() >= 1, "out needs 1 double");
    psamd::bcd_objective(ptr<double>(ym), ym.numel(), ptr<double>(out), cur_stream());
  });
  m.def("bcd_server_stats", [](Tensor w, Tensor active, int64_t c0, int64_t c1, Tensor out) {
    chk(w, at::kDouble, "w");
    chk(active, at::kByte, "active");
    chk(out, at::kDouble, "out");
    check(w.numel() == active.numel(), "w/active mismatch");
    check(0 <= c0 && c0 <= c1 && c1 <= w.numel(), "range outside model");
    check(out.numel() >= 3, "out needs 3 doubles");
    psamd::bcd_server_stats(ptr<double>(w), ptr<uint8_t>(active), c0, c1, ptr<double>(out),
                            cur_stream());
  });

  // ------------------------------------------------------------------ bf16 GEMM
  // C[m,n] = sum_k A(m,k) B(n,k); A(m,k) = A[m*lda+k] if a_kmajor else A[k*lda+m] (B alike)
  m.def("gemm_bf16", [](Tensor A, bool a_kmajor, int64_t lda, Tensor B, bool b_kmajor,
                        int64_t ldb, int64_t M, int64_t N, int64_t K, int epi,
                        optional<Tensor> bias, optional<Tensor> aux, int64_t ldaux,
                        optional<Tensor> C, int64_t ldc, optional<Tensor> Cf, int64_t ldcf,
                        double beta, int splitk, optional<Tensor> colsum) {
    chk(A, at::kBFloat16, "A");
    chk(B, at::kBFloat16, "B");
    check(M > 0 && N > 0 && K > 0 && M < INT32_MAX && N < INT32_MAX && K < INT32_MAX,
          "bad GEMM shape");
    auto need = [&](const Tensor& t, bool kmaj, int64_t ld, int64_t rows, const char* nm) {
      check(ld % 8 == 0, std::string(nm) + ": leading dimension must be a multiple of 8");
      check(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
            std::string(nm) + ": must be 16-byte aligned");
      if (kmaj) {
        check(K % 8 == 0 && ld >= K, std::string(nm) + ": K-major needs K % 8 == 0, ld >= K");
        check(t.numel() >= (rows - 1) * ld + K, std::string(nm) + ": too small");
      } else {
        check(rows % 8 == 0 && ld >= rows, std::string(nm) + ": MN-major needs rows % 8 == 0");
        check(t.numel() >= (K - 1) * ld + rows, std::string(nm) + ": too small");
      }
    };
    need(A, a_kmajor, lda, M, "A");
    need(B, b_kmajor, ldb, N, "B");
    const float* bp = optr<float>(bias, at::kFloat, "bias");
    if (epi & 1) check(bp && bias->numel() >= N, "EPI_BIAS needs bias[N]");
    const void* xp = nullptr;
    if (epi & 4) {
      check(aux.has_value() && aux->defined(), "EPI_MASK needs aux");
      chk(*aux, at::kBFloat16, "aux");
      check(aux->numel() >= (M - 1) * ldaux + N, "aux too small");
      xp = aux->data_ptr();
    }
    void* cp = nullptr;
    if (C.has_value() && C->defined()) {
      chk(*C, at::kBFloat16, "C");
      check(ldc >= N && C->numel() >= (M - 1) * ldc + N, "C too small");
      cp = C->data_ptr();
    }
    float* cfp = optr<float>(Cf, at::kFloat, "Cf");
    if (cfp) check(ldcf >= N && Cf->numel() >= (M - 1) * ldcf + N, "Cf too small");
    check(cp || cfp, "GEMM needs an output");
    if (splitk > 1)
      check(!cp && cfp && (epi & ~8) == 0 && (beta == 0.0 || beta == 1.0),
            "split-K: fp32 output only, no epilogue, beta 0 or 1");
    float* csp = optr<float>(colsum, at::kFloat, "colsum");
    check(!(epi & 8) || (csp && colsum->numel() >= N), "EPI_COLSUM needs colsum[N]");
    psamd::gemm_bf16(a_kmajor, b_kmajor, A.data_ptr(), (int)lda, B.data_ptr(), (int)ldb, (int)M,
                     (int)N, (int)K, epi, bp, xp, (int)ldaux, cp, (int)ldc, cfp, (int)ldcf,
                     (float)beta, splitk, csp, cur_stream());
  });


  // ------------------------------------------------------------- embeddings
  auto rows_check = [](const Tensor& rows, int64_t cap, int D) {
    chk(rows, at::kBFloat16, "rows");
    check(D > 0 && D % 8 == 0 && D <= 128, "embedding dim must be a multiple of 8, <= 128");
    check(rows.dim() == 2 && rows.size(0) == cap && rows.size(1) == D, "rows must be [cap, D]");
  };
  m.def("emb_init_rows", [rows_check](Tensor slot, Tensor keys, optional<Tensor> n_dev,
                                      Tensor rows, Tensor inited, uint64_t seed, double scale) {
    chk(slot, at::kLong, "slot");
    chk(keys, at::kLong, "keys");
    chk(inited, at::kByte, "inited");
    const int64_t cap = inited.numel();
    rows_check(rows, cap, (int)rows.size(1));
    check(keys.numel() >= slot.numel(), "keys shorter than slot");
    psamd::emb_init_rows(ptr<int64_t>(slot), ptr<uint64_t>(keys), slot.numel(),
                         optr<int32_t>(n_dev, at::kInt, "n_dev"), cap, rows.data_ptr(),
                         ptr<uint8_t>(inited), (int)rows.size(1), seed, (float)scale,
                         cur_stream());
  });
  m.def("emb_gather_rows", [rows_check](Tensor slot, Tensor rows, Tensor out,
                                         optional<Tensor> n_dev) {
    // out[i, :] = rows[slot[i], :] for i < n_dev (device count, clamped) or slot.numel()
    chk(slot, at::kLong, "slot");
    rows_check(rows, rows.size(0), (int)rows.size(1));
    chk(out, at::kBFloat16, "out");
    check(out.numel() >= slot.numel() * rows.size(1), "out too small");
    psamd::emb_gather_rows(ptr<int64_t>(slot), slot.numel(), optr<int32_t>(n_dev, at::kInt, "n_dev"),
                           rows.size(0), rows.data_ptr(), (int)rows.size(1), out.data_ptr(),
                           cur_stream());
  }, py::arg("slot"), py::arg("rows"), py::arg("out"), py::arg("n_dev") = py::none());
  m.def("emb_expand", [](Tensor local_col, int64_t nnz, optional<Tensor> idx, Tensor src,
                         Tensor X0) {
    chk(local_col, at::kInt, "local_col");
    chk(src, at::kBFloat16, "src");
    chk(X0, at::kBFloat16, "X0");
    check(src.dim() == 2 && src.size(1) % 8 == 0, "src must be [rows, D], D % 8 == 0");
    const int D = (int)src.size(1);
    check(local_col.numel() >= nnz && X0.numel() >= nnz * D, "expand buffers too small");
    const int64_t* ip = optr<int64_t>(idx, at::kLong, "idx");
    psamd::emb_expand(ptr<int32_t>(local_col), nnz, ip, ip ? idx->numel() : 0, src.data_ptr(),
                      src.size(0), D, X0.data_ptr(), cur_stream());
  });
  // padded (sync-free) exchange of the embedding models; records [C x D bf16 | C f32]
  // per peer chunk (Q = C*D/2 + C int32 words)
  m.def("emb_padded_serve", [](Tensor recv, int64_t H, int64_t C, int kw, Tensor slot, Tensor w,
                               Tensor rows, Tensor inited, int64_t seed, double scale,
                               Tensor out) {
    chk(recv, at::kInt, "recv");
    chk(slot, at::kLong, "slot");
    chk(w, at::kFloat, "w");
    chk(rows, at::kBFloat16, "rows");
    chk(inited, at::kByte, "inited");
    chk(out, at::kInt, "out");
    check(kw == 1 || kw == 2, "kw 1 or 2");
    check(rows.dim() == 2 && rows.size(1) % 8 == 0, "rows [cap, D], D % 8 == 0");
    const int D = (int)rows.size(1);
    check(C > 0 && C % 4 == 0 && H >= 4 + C * kw, "C % 4 == 0, H >= 4 + C kw");
    const int64_t G = recv.numel() / H;
    check(G >= 1 && recv.numel() == G * H, "recv = G rows of H");
    check(slot.numel() >= G * C && w.numel() >= G * C, "slot / w [G*C]");
    check(inited.numel() >= rows.size(0), "inited [cap]");
    check(out.numel() >= G * (C * (D / 2) + C), "out [G * Q]");
    psamd::emb_padded_serve(ptr<int32_t>(recv), H, C, kw, (int)G, ptr<int64_t>(slot),
                            ptr<float>(w), rows.size(0), rows.data_ptr(), ptr<uint8_t>(inited), D,
                            (uint64_t)seed, (float)scale, ptr<int32_t>(out), cur_stream());
  });
  m.def("emb_unpack_records", [](Tensor in, int64_t C, Tensor off, Tensor n_uniq, Tensor rows_u,
                                 Tensor w_u) {
    chk(in, at::kInt, "in");
    chk(off, at::kLong, "off");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(rows_u, at::kBFloat16, "rows_u");
    chk(w_u, at::kFloat, "w_u");
    check(rows_u.dim() == 2 && rows_u.size(1) % 8 == 0, "rows_u [u_cap, D]");
    const int D = (int)rows_u.size(1);
    const int G = (int)off.numel() - 1;
    check(G >= 1 && C > 0 && C % 4 == 0, "off [G+1], C % 4 == 0");
    check(in.numel() >= (int64_t)G * (C * (D / 2) + C), "in [G * Q]");
    check(w_u.numel() >= rows_u.size(0), "w_u [u_cap]");
    psamd::emb_unpack_records(ptr<int32_t>(in), C, G, ptr<int64_t>(off), ptr<int32_t>(n_uniq),
                              rows_u.size(0), D, rows_u.data_ptr(), ptr<float>(w_u),
                              cur_stream());
  });
  m.def("emb_pack_grads", [](Tensor dE, Tensor g_wide, Tensor off, Tensor n_uniq, int64_t C,
                             Tensor out) {
    chk(dE, at::kFloat, "dE");
    chk(g_wide, at::kFloat, "g_wide");
    chk(off, at::kLong, "off");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(out, at::kInt, "out");
    check(dE.dim() == 2 && dE.size(1) % 8 == 0, "dE [u_cap, D]");
    const int D = (int)dE.size(1);
    const int G = (int)off.numel() - 1;
    check(G >= 1 && C > 0 && C % 4 == 0, "off [G+1], C % 4 == 0");
    check(g_wide.numel() >= dE.size(0), "g_wide [u_cap]");
    check(out.numel() >= (int64_t)G * (C * (D / 2) + C), "out [G * Q]");
    psamd::emb_pack_grads(ptr<float>(dE), ptr<float>(g_wide), ptr<int64_t>(off),
                          ptr<int32_t>(n_uniq), dE.size(0), C, G, D, ptr<int32_t>(out),
                          cur_stream());
  });
  m.def("emb_grad_wide_ok", [](int D) { return psamd::emb_grad_wide_ok(D); });
  m.def("emb_grad_reduce", [](Tensor pos_s, Tensor segid, Tensor seg_start, Tensor n_uniq,
                              int64_t u_cap, int64_t nnz, Tensor dX0, int D, Tensor dE,
                              optional<Tensor> coef, int width, optional<Tensor> g_wide) {
    chk(pos_s, at::kInt, "pos_s");
    chk(segid, at::kInt, "segid");
    check(segid.numel() >= nnz, "segid too small");
    chk(seg_start, at::kInt, "seg_start");
    chk(n_uniq, at::kInt, "n_uniq");
    chk(dX0, at::kBFloat16, "dX0");
    chk(dE, at::kFloat, "dE");
    check(D > 0 && D % 8 == 0, "D % 8 == 0");
    check(seg_start.numel() >= u_cap + 1 && pos_s.numel() >= nnz, "segment arrays too small");
    check(dX0.numel() >= nnz * D && dE.numel() >= u_cap * D, "gradient buffers too small");
    // run partials of the segmented wavefront kernels (D = 128 / 256; from the
    // caching allocator, so graph captures keep it in their pool)
    const int64_t pf = psamd::emb_grad_part_floats(nnz, D);
    Tensor part = pf ? at::empty({pf}, dE.options()) : Tensor();
    // wide & deep: g_wide[u] = sum of coef[row] over u's occurrences (row = pos / width)
    const bool wide = g_wide.has_value();
    if (wide) {
      check(coef.has_value() && width > 0 && nnz % width == 0, "g_wide needs coef and width");
      chk(*coef, at::kFloat, "coef");
      chk(*g_wide, at::kFloat, "g_wide");
      check(coef->numel() >= nnz / width && g_wide->numel() >= u_cap, "coef / g_wide too small");
      check(psamd::emb_grad_wide_ok(D), "g_wide rides along only with D = 128 / 256");
    }
    psamd::emb_grad_reduce(ptr<int32_t>(pos_s), ptr<int32_t>(segid), ptr<int32_t>(seg_start),
                           ptr<int32_t>(n_uniq), u_cap, nnz, dX0.data_ptr(), D, ptr<float>(dE),
                           pf ? ptr<float>(part) : nullptr, wide ? ptr<float>(*coef) : nullptr,
                           wide ? width : 0, wide ? ptr<float>(*g_wide) : nullptr, cur_stream());
  }, py::arg("pos_s"), py::arg("segid"), py::arg("seg_start"), py::arg("n_uniq"),
     py::arg("u_cap"), py::arg("nnz"), py::arg("dX0"), py::arg("D"), py::arg("dE"),
     py::arg("coef") = py::none(), py::arg("width") = 0, py::arg("g_wide") = py::none());
  // wide & deep: wide = (slots, g_wide, algo, lr_type, alpha, beta, l1, l2, grad_scale,
  // max_delta) also applies the keys' wide gradients to their table slots (kv_update's
  // update and stats) in the same pass
  m.def("emb_update", [rows_check](Tensor slot, optional<Tensor> n_dev, optional<Tensor> grad,
                                   optional<Tensor> grad16, Tensor rows, Tensor acc, double lr,
                                   double eps, optional<Tensor> slots, optional<Tensor> g_wide,
                                   std::vector<double> rule, optional<Tensor> stats) {
    chk(slot, at::kLong, "slot");
    chk(acc, at::kFloat, "acc");
    const int64_t cap = acc.numel();
    const int D = (int)rows.size(1);
    rows_check(rows, cap, D);
    const float* gp = optr<float>(grad, at::kFloat, "grad");
    const void* g16 = nullptr;
    if (!gp) {
      check(grad16.has_value() && grad16->defined(), "emb_update needs grad or grad16");
      chk(*grad16, at::kBFloat16, "grad16");
      check(grad16->numel() >= slot.numel() * D, "grad16 too small");
      g16 = grad16->data_ptr();
    } else {
      check(grad->numel() >= slot.numel() * D, "grad too small");
    }
    void* sp = nullptr;
    const float* gw = nullptr;
    int wr[2] = {0, 0};
    float wh[6] = {0, 0, 0, 0, 0, 0};
    if (slots.has_value()) {
      check(slot_capacity(*slots) == cap, "emb_update: slots and rows must be one table");
      chk(*g_wide, at::kFloat, "g_wide");
      check(g_wide->numel() >= slot.numel(), "g_wide too small");
      check(rule.size() == 8, "wide rule = algo, lr_type, alpha, beta, l1, l2, grad_scale, max_delta");
      check(rule[2] > 0, "learning rate alpha must be > 0");
      sp = slots->data_ptr();
      gw = ptr<float>(*g_wide);
      wr[0] = (int)rule[0];
      wr[1] = (int)rule[1];
      for (int q = 0; q < 6; ++q) wh[q] = (float)rule[2 + q];
    }
    psamd::emb_update(ptr<int64_t>(slot), slot.numel(), optr<int32_t>(n_dev, at::kInt, "n_dev"),
                      cap, gp, g16, rows.data_ptr(), ptr<float>(acc), D, (float)lr, (float)eps, sp,
                      gw, wr, wh, optr<double>(stats, at::kDouble, "stats"), acc_stripes_of(stats),
                      cur_stream());
  }, py::arg("slot"), py::arg("n_dev"), py::arg("grad"), py::arg("grad16"), py::arg("rows"),
     py::arg("acc"), py::arg("lr"), py::arg("eps"), py::arg("slots") = py::none(),
     py::arg("g_wide") = py::none(), py::arg("rule") = std::vector<double>{},
     py::arg("stats") = py::none());
  m.def("wd_head", [](Tensor h, Tensor w, Tensor b, Tensor wide_w, Tensor local_col, int S,
                      Tensor labels, Tensor coef, Tensor dh, Tensor dw, Tensor db, Tensor metrics,
                      Tensor hist, int nbins, optional<Tensor> db_h) {
    chk(h, at::kBFloat16, "h");
    chk(w, at::kFloat, "w");
    chk(b, at::kFloat, "b");
    chk(wide_w, at::kFloat, "wide_w");
    chk(local_col, at::kInt, "local_col");
    chk(labels, at::kFloat, "labels");
    chk(coef, at::kFloat, "coef");
    chk(dh, at::kBFloat16, "dh");
    chk(dw, at::kFloat, "dw");
    chk(db, at::kFloat, "db");
    chk(metrics, at::kDouble, "metrics");
    chk(hist, at::kInt, "hist");
    check(h.dim() == 2, "h must be [B, H]");
    const int64_t B = h.size(0);
    const int H = (int)h.size(1);
    check(H > 0 && H <= 512 && w.numel() == H && dw.numel() == H, "head width H in (0, 512]");
    check(S > 0 && S <= 64 && local_col.numel() >= B * S, "S in (0, 64], local_col [B*S]");
    check(labels.numel() >= B && coef.numel() >= B && dh.numel() >= B * H, "head buffers small");
    check(metrics.numel() >= 3 && hist.numel() >= 2 * nbins && nbins > 0, "metrics / hist");
    float* dbh = optr<float>(db_h, at::kFloat, "db_h");
    check(!dbh || db_h->numel() >= H, "db_h [H]");
    check(H % 8 == 0, "head width H % 8 == 0");
    psamd::wd_head(h.data_ptr(), B, H, ptr<float>(w), ptr<float>(b), ptr<float>(wide_w),
                   wide_w.numel(), ptr<int32_t>(local_col), S, ptr<float>(labels),
                   ptr<float>(coef), dh.data_ptr(), ptr<float>(dw), ptr<float>(db), dbh,
                   ptr<double>(metrics), reinterpret_cast<uint32_t*>(hist.data_ptr()), nbins,
                   acc_stripes_of(metrics), cur_stream());
  });
  m.def("colsum_bf16", [](Tensor x, Tensor out) {
    chk(x, at::kBFloat16, "x");
    chk(out, at::kFloat, "out");
    check(x.dim() == 2 && out.numel() >= x.size(1), "colsum: x [B, N], out [N]");
    check(x.size(1) % 8 == 0, "colsum: N % 8 == 0");
    psamd::colred_bf16(x.data_ptr(), x.size(0), (int)x.size(1), nullptr, ptr<float>(out), nullptr,
                       nullptr, cur_stream());
  });
  m.def("adam_update", [](Tensor p, Tensor g, Tensor m_, Tensor v, double lr, double b1,
                          double b2, double eps, int64_t step, double gscale,
                          optional<Tensor> p16, optional<Tensor> step_dev, bool zero_grad) {
    chk(p, at::kFloat, "p");
    chk(g, at::kFloat, "g");
    chk(m_, at::kFloat, "m");
    chk(v, at::kFloat, "v");
    const int64_t n = p.numel();
    check(g.numel() == n && m_.numel() == n && v.numel() == n, "adam buffers mismatch");
    void* p16p = nullptr;
    if (p16.has_value() && p16->defined()) {
      chk(*p16, at::kBFloat16, "p16");
      check(p16->numel() == n, "p16 mismatch");
      p16p = p16->data_ptr();
    }
    const int64_t* sd = nullptr;  // device step clock (graph-captured steps)
    if (step_dev.has_value() && step_dev->defined()) {
      chk(*step_dev, at::kLong, "step_dev");
      sd = step_dev->data_ptr<int64_t>();
    } else {
      check(step >= 1, "adam step >= 1");
    }
    const double s1 = (double)(step >= 1 ? step : 1);
    const double bc1 = 1.0 - std::pow(b1, s1), bc2 = 1.0 - std::pow(b2, s1);
    psamd::adam_update(ptr<float>(p), ptr<float>(g), ptr<float>(m_), ptr<float>(v), n, (float)lr,
                       (float)b1, (float)b2, (float)eps, (float)bc1, (float)bc2, (float)gscale,
                       p16p, sd, zero_grad, cur_stream());
  });
  // SparseMatrix::times (utils/matrix.py): gather (row-reduce) or scatter (atomic) over the
  // compressed major dimension; y = alpha * A x + beta * y.
  m.def("spmv", [](bool scatter, Tensor off, Tensor idx, optional<Tensor> val, Tensor x, Tensor y,
                   double alpha, double beta) {
    chk(off, at::kLong, "offset");
    check(idx.is_cuda() && idx.is_contiguous() &&
              (idx.scalar_type() == at::kInt || idx.scalar_type() == at::kLong),
          "spmv: index must be contiguous int32/int64 on the GPU");
    check(x.is_cuda() && x.is_contiguous() &&
              (x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble),
          "spmv: x must be contiguous float32/float64 on the GPU");
    chk(y, x.scalar_type(), "y");
    const int64_t n_major = off.numel() - 1, nnz = idx.numel();
    check(n_major >= 0, "spmv: offset must have n_major + 1 entries");
    const void* vp = nullptr;
    if (val.has_value() && val->defined()) {
      chk(*val, x.scalar_type(), "value");
      check(val->numel() == nnz, "spmv: value / index length mismatch");
      vp = val->data_ptr();
    }
    if (scatter) check(x.numel() >= n_major, "spmv(scatter): x shorter than the major dimension");
    else check(y.numel() >= n_major, "spmv(gather): y shorter than the major dimension");
    psamd::spmv(scatter, ptr<int64_t>(off), idx.data_ptr(), (int)idx.element_size(), vp,
                (int)x.element_size(), n_major, nnz, x.data_ptr(), x.numel(), alpha, beta,
                y.data_ptr(), y.numel(), cur_stream());
  });
}

PYBIND11_MODULE(_hipops, m) {
  m.doc() = "parameter_server_amd HIP kernels (gfx950)";
  register_launch(m);
  register_table(m);
  register_tploc(m);
  register_prep(m);
  register_linear(m);
  register_dense(m);
  register_scoretext(m);
  register_slotsplit(m);
}
