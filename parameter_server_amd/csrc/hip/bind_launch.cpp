// The launch unit of the _hipops bindings: LaunchList, GraphChain and the raw event
// helpers. The kernel ops' LaunchList.add_* methods come from the units that own them.
#include "bind_common.h"

using namespace psamd_bind;

namespace {

// A linear HIP graph composed natively: child graphs (torch CUDAGraphs captured with
// keep_graph=True, cloned in) and event wait / record nodes, chained in order. One launch
// replays a stream's whole iteration with its cross-stream event edges in the graph
// (bench.py's merged pipeline, PSAMD_MX_G2; benchmarks/probe_graph_events.py).
struct GraphChain {
  hipGraph_t g = nullptr;
  hipGraphExec_t ex = nullptr;
  hipGraphNode_t last = nullptr;
  std::vector<py::object> keep;
  GraphChain() { PSAMD_HIP_CHECK(hipGraphCreate(&g, 0)); }
  ~GraphChain() {
    if (ex) (void)hipGraphExecDestroy(ex);
    if (g) (void)hipGraphDestroy(g);
  }
  GraphChain(const GraphChain&) = delete;
  GraphChain& operator=(const GraphChain&) = delete;
  void chain(hipGraphNode_t n) { last = n; }
  const hipGraphNode_t* deps() const { return last ? &last : nullptr; }
  size_t ndeps() const { return last ? 1 : 0; }
};

hipEvent_t list_event(const py::object& ev, const char* what) {
  const uint64_t v = py::isinstance<py::int_>(ev) ? ev.cast<uint64_t>()
                                                  : ev.attr("cuda_event").cast<uint64_t>();
  check(v != 0, std::string(what) + ": event not created yet (record it once first)");
  return reinterpret_cast<hipEvent_t>(v);
}

}  // namespace

void psamd_bind::register_launch(py::module_& m) {
  // raw HIP events for native launch lists (handle as an integer; the caller destroys it)
  m.def("event_create", []() {
    hipEvent_t e = nullptr;
    PSAMD_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return reinterpret_cast<uint64_t>(e);
  });
  m.def("event_destroy", [](uint64_t e) {
    if (e) PSAMD_HIP_CHECK(hipEventDestroy(reinterpret_cast<hipEvent_t>(e)));
  });

  py::class_<GraphChain>(m, "GraphChain")
      .def(py::init<>())
      .def("add_child", [](GraphChain& c, py::object torch_graph) {
        check(c.ex == nullptr, "GraphChain: already instantiated");
        const py::object h = torch_graph.attr("raw_cuda_graph")();
        const hipGraph_t child = reinterpret_cast<hipGraph_t>(h.cast<uint64_t>());
        check(child != nullptr, "GraphChain.add_child: capture with keep_graph=True");
        hipGraphNode_t n;
        PSAMD_HIP_CHECK(hipGraphAddChildGraphNode(&n, c.g, c.deps(), c.ndeps(), child));
        c.chain(n);
        c.keep.push_back(torch_graph);
      })
      .def("add_wait", [](GraphChain& c, py::object event) {
        check(c.ex == nullptr, "GraphChain: already instantiated");
        hipGraphNode_t n;
        PSAMD_HIP_CHECK(hipGraphAddEventWaitNode(&n, c.g, c.deps(), c.ndeps(),
                                                 list_event(event, "GraphChain.add_wait")));
        c.chain(n);
        c.keep.push_back(event);
      })
      .def("add_record", [](GraphChain& c, py::object event) {
        check(c.ex == nullptr, "GraphChain: already instantiated");
        hipGraphNode_t n;
        PSAMD_HIP_CHECK(hipGraphAddEventRecordNode(&n, c.g, c.deps(), c.ndeps(),
                                                   list_event(event, "GraphChain.add_record")));
        c.chain(n);
        c.keep.push_back(event);
      })
      .def("instantiate", [](GraphChain& c) {
        if (!c.ex) PSAMD_HIP_CHECK(hipGraphInstantiate(&c.ex, c.g, nullptr, nullptr, 0));
      })
      .def("launch", [](GraphChain& c) {
        check(c.ex != nullptr, "GraphChain: instantiate first");
        PSAMD_HIP_CHECK(hipGraphLaunch(c.ex, cur_stream()));
      })
      // (like CUDAGraph.reset: frees the executable graph; the caller synchronised)
      .def("reset", [](GraphChain& c) {
        if (c.ex) PSAMD_HIP_CHECK(hipGraphExecDestroy(c.ex));
        c.ex = nullptr;
        c.keep.clear();
      });

  // A validate-once launch list: the add_* calls check their arguments exactly as the
  // single ops and keep the tensors alive; run() issues every launch in order on the
  // current stream with no per-call argument conversion. The 1-GPU sparse-LR step
  // (resolve, fused forward + backward, fused scan + update) runs from one per
  // minibatch buffer: three pybind crossings with 60 tensor / scalar arguments cost
  // ~10 us of host issue time per step (profiles/r3_s3_host_issue.log). The kernel ops'
  // add_* methods come from the units that own them (def_launch, bind_common.h).
  py::class_<LaunchList>(m, "LaunchList")
      .def(py::init<>())
      .def("add_chain", [](LaunchList& l, py::object chain) {
        GraphChain& c = chain.cast<GraphChain&>();
        check(c.ex != nullptr, "add_chain: instantiate the GraphChain first");
        const hipGraphExec_t ex = c.ex;
        l.keep.push_back(chain);
        l.push_op([ex](hipStream_t& s) { PSAMD_HIP_CHECK(hipGraphLaunch(ex, s)); }, "chain");
      })
      // control ops: a torch.cuda.Stream / torch.cuda.Event (the list keeps a reference:
      // a torch Event destroys its HIP event with the object, and a raw handle left in a
      // list then fails on the next run) or a raw handle the caller owns (event_create).
      // Events must exist already (torch creates them lazily: record once first).
      .def("add_stream", [](LaunchList& l, py::object stream) {
        const uint64_t v = py::isinstance<py::int_>(stream)
                               ? stream.cast<uint64_t>()
                               : stream.attr("cuda_stream").cast<uint64_t>();
        const hipStream_t h = reinterpret_cast<hipStream_t>(v);
        l.keep.push_back(stream);
        l.push_op([h](hipStream_t& s) { s = h; }, "stream");
      })
      .def("add_wait", [](LaunchList& l, py::object event) {
        const hipEvent_t e = list_event(event, "add_wait");
        l.keep.push_back(event);
        l.push_op([e](hipStream_t& s) { PSAMD_HIP_CHECK(hipStreamWaitEvent(s, e, 0)); }, "wait");
      })
      .def("add_record", [](LaunchList& l, py::object event) {
        const hipEvent_t e = list_event(event, "add_record");
        l.keep.push_back(event);
        l.push_op([e](hipStream_t& s) { PSAMD_HIP_CHECK(hipEventRecord(e, s)); }, "record");
      })
      // replay of a captured torch.cuda.CUDAGraph (the list keeps the graph alive):
      // hipGraphLaunch of its executable graph on the list's current stream. Only for
      // graphs whose kernels draw nothing from torch's RNG (torch's replay() also
      // advances the captured generator offsets; ours use their own counters)
      .def("add_graph", [](LaunchList& l, py::object graph) {
        const py::object h = graph.attr("raw_cuda_graph_exec")();
        if (!py::isinstance<py::int_>(h))
          throw std::invalid_argument("add_graph: raw_cuda_graph_exec() is not an int handle");
        const hipGraphExec_t ex = reinterpret_cast<hipGraphExec_t>(h.cast<uint64_t>());
        if (!ex) throw std::invalid_argument("add_graph: graph not instantiated");
        l.keep.push_back(graph);
        l.push_op([ex](hipStream_t& s) { PSAMD_HIP_CHECK(hipGraphLaunch(ex, s)); }, "graph");
      })
      // the ops of another list, SHARED (a generator's row cursor advances for both)
      .def("extend", [](LaunchList& l, const LaunchList& o) {
        l.ops.insert(l.ops.end(), o.ops.begin(), o.ops.end());
        l.names.insert(l.names.end(), o.names.begin(), o.names.end());
        l.keep.insert(l.keep.end(), o.keep.begin(), o.keep.end());
      })
      .def("__len__", [](const LaunchList& l) { return l.ops.size(); })
      .def("run", [](const LaunchList& l) {
        hipStream_t st = cur_stream();
        size_t i = 0;
        try {
          for (; i < l.ops.size(); ++i) l.ops[i](st);
        } catch (const std::exception& e) {
          throw std::runtime_error("LaunchList op " + std::to_string(i) + " of " +
                                   std::to_string(l.ops.size()) + " (" + l.names[i] +
                                   "): " + e.what());
        }
      });
}
