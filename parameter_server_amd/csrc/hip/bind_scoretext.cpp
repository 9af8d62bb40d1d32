// Bindings of the prediction-line formatter (scoretext.hip).
#include "bind_common.h"
#include "scoretext.h"

using namespace psamd_bind;

void psamd_bind::register_scoretext(py::module_& m) {
  m.def("scoretext_block", [] { return psamd::scoretext_block(); });
  m.def("scoretext_max_line", [](int ncols) {
    check(ncols == 1 || ncols == 2, "scoretext_max_line: one or two columns");
    return psamd::scoretext_max_line(ncols);
  });
  m.def("scoretext_work_bytes", [](int64_t n) {
    check(n >= 0, "scoretext_work_bytes: negative row count");
    return psamd::scoretext_work_bytes(n);
  });
  // Lines "first\n" or "first\tsecond\n" of the first n = first.numel() rows into
  // out[:cap] (cap < 0: all of out); hdr = {text bytes, deferred values, over capacity}.
  m.def("scoretext_format", [](Tensor first, optional<Tensor> second, Tensor out, Tensor hdr,
                               Tensor work, int64_t cap) {
    chk(first, at::kFloat, "first");
    chk(out, at::kByte, "out");
    chk(hdr, at::kLong, "hdr");
    chk(work, at::kByte, "work");
    const int64_t n = first.numel();
    const float* sp = optr<float>(second, at::kFloat, "second");
    if (sp) check(second->numel() == n, "scoretext_format: the columns must be equally long");
    if (cap < 0) cap = out.numel();
    check(cap <= out.numel(), "scoretext_format: cap beyond the output buffer");
    check(hdr.numel() >= 3, "scoretext_format: header needs 3 words");
    check(work.numel() >= psamd::scoretext_work_bytes(n), "scoretext_format: work buffer too small");
    psamd::scoretext_format(reinterpret_cast<const uint32_t*>(ptr<float>(first)),
                            reinterpret_cast<const uint32_t*>(sp), n, ptr<uint8_t>(out), cap,
                            ptr<int64_t>(hdr), ptr<uint8_t>(work), cur_stream());
  }, py::arg("first"), py::arg("second"), py::arg("out"), py::arg("hdr"), py::arg("work"),
     py::arg("cap") = -1);
}
