// binding_common.cpp -- what the bodies of the Python binding share: the DLPack capsule, the argument readers, the shape rules.
#include "binding_common.h"

namespace gbrl_py {
namespace {

// ---- DLPack ABI (public spec, "dltensor" capsule protocol) -- the minimal declarations needed to hand a buffer over
enum { kDLCPU_ = 1, kDLROCM_ = 10 };
struct DLDevice_ { int32_t device_type; int32_t device_id; };
struct DLDataType_ { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DLTensor_ {
    void *data; DLDevice_ device; int32_t ndim; DLDataType_ dtype; int64_t *shape; int64_t *strides; uint64_t byte_offset;
};
struct DLManagedTensor_ {
    DLTensor_ dl_tensor; void *manager_ctx; void (*deleter)(DLManagedTensor_ *);
};

void dl_deleter(DLManagedTensor_ *self) {
    if (self->dl_tensor.device.device_type == kDLROCM_) gbrl_hip_device_free(self->dl_tensor.data);
    else delete[] static_cast<float *>(self->dl_tensor.data);
    delete[] self->dl_tensor.shape;
    delete self;
}

void capsule_destructor(PyObject *cap) {
    // an unconsumed capsule still owns the tensor (consumers rename it to "used_dltensor")
    if (PyCapsule_IsValid(cap, "dltensor")) {
        auto *mt = static_cast<DLManagedTensor_ *>(PyCapsule_GetPointer(cap, "dltensor"));
        if (mt && mt->deleter) mt->deleter(mt);
    }
}

}  // namespace

py::object make_dlpack(void *data, const std::vector<int64_t> &shape, bool on_device, int device_id, bool int32) {
    auto *mt = new DLManagedTensor_;
    mt->dl_tensor.data = data;
    mt->dl_tensor.device = {on_device ? kDLROCM_ : kDLCPU_, on_device ? device_id : 0};
    mt->dl_tensor.ndim = static_cast<int32_t>(shape.size());
    mt->dl_tensor.dtype = {static_cast<uint8_t>(int32 ? 0 /*kDLInt*/ : 2 /*kDLFloat*/), 32, 1};
    mt->dl_tensor.shape = new int64_t[shape.size()];
    std::copy(shape.begin(), shape.end(), mt->dl_tensor.shape);
    mt->dl_tensor.strides = nullptr;
    mt->dl_tensor.byte_offset = 0;
    mt->manager_ctx = nullptr;
    mt->deleter = dl_deleter;
    return py::reinterpret_steal<py::object>(PyCapsule_New(mt, "dltensor", capsule_destructor));
}

[[noreturn]] void fail(const std::string &msg) { throw std::runtime_error(msg); }
void check(int status) {
    if (status != GBRL_HIP_OK) fail(gbrl_hip_last_error());
}

// handle_input_info (binding.cpp:156-190): None | NumPy array | (data_ptr, shape, dtype, device)
// `categorical`: 0 = float32 values, 1 = 128-byte cells, 2 = int32 dictionary ids (encode_categorical / predict_encoded, an extension)
Input read_input(py::object &obj, const std::string &name, bool none_allowed, const std::string &fn, int categorical) {
    Input in;
    if (obj.is_none()) {
        if (!none_allowed) fail("Cannot call " + fn + " without " + name + "!");
        return in;
    }
    if (py::isinstance<py::array>(obj)) {
        py::array arr = py::array::ensure(obj, py::array::c_style | py::array::forcecast);
        if (!arr) fail("Could not convert object to a contiguous NumPy array");
        py::buffer_info info = arr.request();
        const std::string want = categorical == 1 ? "128s" : categorical == 2 ? py::format_descriptor<int32_t>::format() : py::format_descriptor<float>::format();
        if (info.format != want) fail_cat("Expected array of format '", want, "', but got '", info.format, "'");
        in.ptr = info.ptr;
        in.shape.assign(info.shape.begin(), info.shape.end());
        in.keep = arr;
        return in;
    }
    if (py::isinstance<py::tuple>(obj)) {
        py::tuple t = obj.cast<py::tuple>();
        if (t.size() != 4) fail("Expected a tuple of size 4: (data_ptr, shape, dtype, device)");
        const uintptr_t raw = t[0].cast<uintptr_t>();
        in.ptr = (raw == 0 || raw == static_cast<uintptr_t>(-1)) ? nullptr : reinterpret_cast<const void *>(raw);
        for (py::handle d : t[1].cast<py::tuple>()) in.shape.push_back(d.cast<size_t>());
        const std::string dtype = t[2].cast<std::string>();
        if (categorical == 2) {
            if (dtype != "torch.int32") fail("Expected dtype torch.int32, but got " + dtype);
        } else if (categorical) {
            // extension over the reference (which takes categorical cells as NumPy S128 arrays only): a device-resident cell
            // matrix, [n, n_cat] cells of 128 bytes each (e.g. a torch.uint8 tensor [n, n_cat, 128]), announced as dtype "S128"
            if (dtype != "S128" && dtype != "|S128") fail("Unsupported data type: " + dtype);
        } else if (dtype != "torch.float32") {
            fail("Expected dtype torch.float32, but got " + dtype);
        }
        const std::string dev = t[3].cast<std::string>();
        if (dev == "cpu") in.on_device = false;
        else if (dev == "cuda" || dev == "gpu") in.on_device = true;
        else fail("Invalid device! Options are: cpu/cuda");
        return in;
    }
    fail("Unknown " + name + " type! Must be a NumPy array or tuple.");
}

int parse_enum(const std::string &s, std::initializer_list<std::pair<const char *, int>> opts, const char *err) {
    for (const auto &o : opts)
        if (s == o.first) return o.second;
    fail(err);
}
int parse_device(const std::string &s) {  // stringTodeviceType, types.cpp:58-62
    return parse_enum(s, {{"cpu", 0}, {"cuda", 1}, {"gpu", 1}}, "Invalid device! Options are: cpu/cuda");
}

// parity mode names of GBRL(parity_mode=...), set_parity_mode and get_parity_mode (gbrl_hip_parity_mode, include/gbrl_hip.h)
int parse_parity_mode(const std::string &s) {
    return parse_enum(s, {{"default", GBRL_HIP_PARITY_DEFAULT}, {"reference", GBRL_HIP_PARITY_REFERENCE}, {"exact_argmax", GBRL_HIP_PARITY_EXACT_ARGMAX}},
                      "Invalid parity mode! Options are: default/reference/exact_argmax");
}
// objective names of fit_prepared(objective=), objective_gradient and objective_gradient_host (GBRL_HIP_OBJ_*, include/gbrl_hip.h)
int parse_objective(const std::string &s) {
    return parse_enum(s, {{"rmse", GBRL_HIP_OBJ_RMSE}, {"logistic", GBRL_HIP_OBJ_LOGISTIC}, {"softmax", GBRL_HIP_OBJ_SOFTMAX}, {"quantile", GBRL_HIP_OBJ_QUANTILE},
                          {"pairwise", GBRL_HIP_OBJ_PAIRWISE}, {"lambdarank", GBRL_HIP_OBJ_LAMBDARANK}},
                      "Invalid objective! Options are: rmse/logistic/softmax/quantile/pairwise/lambdarank");
}
// metric names of fit_prepared(eval_metric=), eval_metric and eval_metric_host (GBRL_HIP_METRIC_*, include/gbrl_hip.h)
int parse_metric(const std::string &s) {
    return parse_enum(s, {{"error", GBRL_HIP_METRIC_ERROR}, {"auc", GBRL_HIP_METRIC_AUC}}, "Invalid metric! Options are: error/auc");
}
// leaf rule names of fit_prepared(leaf_update=) (GBRL_HIP_LEAF_*, include/gbrl_hip.h)
int parse_leaf_update(const std::string &s) {
    return parse_enum(s, {{"gradient", GBRL_HIP_LEAF_GRADIENT}, {"newton", GBRL_HIP_LEAF_NEWTON}, {"quantile", GBRL_HIP_LEAF_QUANTILE}},
                      "Invalid leaf_update! Options are: gradient/newton/quantile");
}
const char *parity_mode_name(int mode) {
    return mode == GBRL_HIP_PARITY_REFERENCE ? "reference" : (mode == GBRL_HIP_PARITY_EXACT_ARGMAX ? "exact_argmax" : "default");
}

Input require_input(py::object &obj, const std::string &name, const std::string &fn, int categorical) {
    Input in = read_input(obj, name, false, fn, categorical);
    if (!in.ptr) fail("Cannot call " + fn + " without " + name + "!");
    return in;
}

void require_host(const Input &in, const std::string &text) {
    if (in.on_device) fail(text);
}

const gbrl_hip_dataset *dataset_handle(py::object &ds_obj) { return ds_obj.is_none() ? nullptr : ds_obj.cast<const PyDataset &>().h; }
gbrl_hip_dataset_desc dataset_info(py::object &ds_obj) { return ds_obj.is_none() ? gbrl_hip_dataset_desc{} : ds_obj.cast<const PyDataset &>().info(); }

TreeRange read_tree_range(py::object &start_obj, py::object &stop_obj) {
    return {start_obj.is_none() ? 0 : start_obj.cast<int>(), stop_obj.is_none() ? 0 : stop_obj.cast<int>()};
}

int result_device(PyGBRL &self, bool on_device) {
    if (!on_device) return 0;
    const int id = gbrl_hip_device_ordinal(self.h);
    if (id < 0) fail(gbrl_hip_last_error());
    return id;
}

void one_dim_obs(size_t len, int in_dim, int &n, int &n_features) {
    if (static_cast<int>(len) == in_dim) { n = 1; n_features = in_dim; } else { n = static_cast<int>(len); n_features = 1; }
}

OutputRows read_output_rows(const Input &a, int output_dim, const char *noun) {   // binding.cpp:462-478, 541-556
    int n, dim;
    if (a.shape.size() == 1) {
        if (output_dim > 1) { n = 1; dim = static_cast<int>(a.shape[0]); } else { n = static_cast<int>(a.shape[0]); dim = 1; }
    } else { n = static_cast<int>(a.shape[0]); dim = static_cast<int>(a.shape[1]); }
    if (dim != output_dim) fail_cat(noun, " output dim ", dim, " != correct output dim ", output_dim);
    return {n, dim};
}

BatchShape infer_batch(const Input &o, const Input &c, int in_dim) {
    int n = 0, n_num = 0, n_cat = 0;
    auto neq = [&](size_t a, size_t b) {
        if (a != b) fail_cat("Number of samples is not equal between obs and categorical obs ", a, " != ", b);
    };
    if (o.ptr && c.ptr) {
        if (o.shape.size() == 1 && c.shape.size() == 1) {
            if (static_cast<int>(o.shape[0] + c.shape[0]) == in_dim) { n = 1; n_num = static_cast<int>(o.shape[0]); n_cat = static_cast<int>(c.shape[0]); }
            else { neq(o.shape[0], c.shape[0]); n = static_cast<int>(o.shape[0]); n_num = 1; n_cat = 1; }
        } else if (o.shape.size() == 1) { neq(o.shape[0], c.shape[0]); n = static_cast<int>(o.shape[0]); n_num = 1; n_cat = static_cast<int>(c.shape[1]);
        } else if (c.shape.size() == 1) { neq(o.shape[0], c.shape[0]); n = static_cast<int>(o.shape[0]); n_num = static_cast<int>(o.shape[1]); n_cat = 1;
        } else { neq(o.shape[0], c.shape[0]); n = static_cast<int>(o.shape[0]); n_num = static_cast<int>(o.shape[1]); n_cat = static_cast<int>(c.shape[1]); }
    } else if (o.ptr) {
        if (o.shape.size() == 1) one_dim_obs(o.shape[0], in_dim, n, n_num);
        else { n = static_cast<int>(o.shape[0]); n_num = static_cast<int>(o.shape[1]); }
    } else {
        if (c.shape.size() == 1) one_dim_obs(c.shape[0], in_dim, n, n_cat);
        else { n = static_cast<int>(c.shape[0]); n_cat = static_cast<int>(c.shape[1]); }
    }
    if (n_num + n_cat != in_dim) fail_cat("Total number of features ", n_num + n_cat, " != input dim ", in_dim);
    return {n, n_num, n_cat};
}

Batch read_batch(py::object &obs, py::object &cat, const std::string &fn, int in_dim, bool ids, py::object *extra, const char *extra_name) {
    Batch b;
    b.o = read_input(obs, "obs", true, fn, false);
    b.c = read_input(cat, "cat_obs", true, fn, ids ? 2 : 1);
    if (!b.o.ptr && !b.c.ptr) fail("Cannot call " + fn + " without observations!");
    if (extra) b.extra = require_input(*extra, extra_name, fn);
    b.s = infer_batch(b.o, b.c, in_dim);
    return b;
}

// `a` (base or targets) is [n, D], or [n] when D == 1
void check_rows_by_outputs(const Input &a, const char *name, int n, int D) {
    const bool shape_ok = (a.shape.size() == 2 && a.shape[0] == static_cast<size_t>(n) && a.shape[1] == static_cast<size_t>(D)) ||
                          (a.shape.size() == 1 && D == 1 && a.shape[0] == static_cast<size_t>(n));
    if (shape_ok) return;
    std::stringstream ss;
    ss << "Expected " << name << " of shape (" << n << ", " << D << ")" << (D == 1 ? " or (" + std::to_string(n) + ",)" : std::string()) << ", but got (";
    for (size_t i = 0; i < a.shape.size(); ++i) ss << (i ? ", " : "") << a.shape[i];
    ss << ")";
    fail(ss.str());
}

std::vector<int32_t> read_stops(py::object &stops_obj, int n_trees) {
    std::vector<int32_t> stops;
    if (stops_obj.is_none()) {
        for (int k = 1; k <= n_trees; ++k) stops.push_back(k);
    } else {
        for (py::handle k : py::iter(stops_obj)) stops.push_back(k.cast<int32_t>());
    }
    // the engine checks the same (c_api callers); here too because a "cuda" model allocates its result on the device before the C call
    if (stops.empty()) fail("stops is empty: nothing to evaluate");
    for (size_t i = 0; i < stops.size(); ++i) {
        if (stops[i] < 0 || stops[i] > n_trees) fail_cat("a stop is out of bounds! Got ", stops[i], ", but valid range is [0, ", n_trees, "]");
        if (i > 0 && stops[i] <= stops[i - 1]) fail("stops must be strictly ascending");
    }
    return stops;
}

// rows=None | int32 NumPy vector | (data_ptr, (m,), "torch.int32", device)
Input read_rows(py::object &rows, const std::string &fn) {
    Input r = read_input(rows, "rows", true, fn, 2);
    if (!rows.is_none() && !r.ptr && !(r.shape.size() == 1 && r.shape[0] == 0)) fail("Cannot call " + fn + " with a null rows pointer!");
    if (!rows.is_none() && r.shape.size() != 1) fail("rows must be a one-dimensional int32 vector");
    return r;
}

RowsArg read_rows_arg(py::object &rows, const std::string &fn, py::object &ds_obj, const Input &first) {
    static const int32_t kNoRows = 0;   // an empty rows vector is "m == 0", not "every row"
    const Input r = read_rows(rows, fn);
    int m = first.shape.empty() ? 0 : static_cast<int>(first.shape[0]);
    if (!rows.is_none()) m = static_cast<int>(r.shape[0]);
    else if (!ds_obj.is_none()) m = ds_obj.cast<const PyDataset &>().info().n_rows;
    return {rows.is_none() ? nullptr : (r.ptr ? r.i32() : &kNoRows), r.ptr ? r.on_device : 0, m};
}

// cols=: a one-dimensional vector of column indices in host memory (a NumPy integer array or a sequence of ints); the C ABI checks its contents
std::vector<int32_t> read_cols(py::object &cols, const std::string &fn) {
    py::array any = py::array::ensure(cols);
    if (!any) { PyErr_Clear(); fail(fn + ": cols must be a vector of integers"); }
    if (any.ndim() != 1) fail(fn + ": cols must be one-dimensional");
    if (any.size() == 0) return {};   // (an empty list has no integer dtype; the caller refuses "no column")
    if (any.dtype().kind() != 'i' && any.dtype().kind() != 'u') fail(fn + ": cols must be a vector of integers");
    auto a = py::array_t<int64_t, py::array::c_style | py::array::forcecast>::ensure(any);
    if (!a) { PyErr_Clear(); fail(fn + ": cols must be a vector of integers"); }
    std::vector<int32_t> out(static_cast<size_t>(a.shape(0)));
    for (size_t i = 0; i < out.size(); ++i) {
        const int64_t v = a.at(static_cast<py::ssize_t>(i));
        out[i] = v < INT32_MIN ? INT32_MIN : v > INT32_MAX ? INT32_MAX : static_cast<int32_t>(v);   // (out of any range either way)
    }
    return out;
}

// the targets of an objective: float32 [n, D] ([n] when D == 1) for rmse and logistic, int32 [n] labels for softmax
Input read_objective_targets(py::object &targets, const char *name, bool none_allowed, const std::string &fn, int objective, int n, int D, bool check_shape) {
    const bool ranking = objective == GBRL_HIP_OBJ_PAIRWISE || objective == GBRL_HIP_OBJ_LAMBDARANK;   // int32 relevance labels [n]
    if (objective != GBRL_HIP_OBJ_SOFTMAX && !ranking) {
        Input t = read_input(targets, name, none_allowed, fn, false);
        if (check_shape && t.ptr) check_rows_by_outputs(t, name, n, D);
        return t;
    }
    Input t = read_input(targets, name, none_allowed, fn, 2);
    if (check_shape && t.ptr && !(t.shape.size() == 1 && t.shape[0] == static_cast<size_t>(n))) {
        fail_cat("Expected ", name, " of the ", (ranking ? "ranking objective as int32 relevance labels" : "softmax objective as int32 class labels"), " of shape (", n, ",)");
    }
    return t;
}

// row weights (include/gbrl_hip.h, "Row weights"): None, or float32 [n] as a NumPy array or a device tuple
Input read_weights(py::object &weights, const char *name, const std::string &fn, int n, bool check_shape) {
    if (weights.is_none()) return Input{};
    Input w = read_input(weights, name, false, fn, false);
    if (!w.ptr) fail("Cannot call " + fn + " with a null " + name + " pointer!");
    if (check_shape && !(w.shape.size() == 1 && w.shape[0] == static_cast<size_t>(n))) {
        fail_cat("Expected ", name, " as a float32 vector of shape (", n, ",), one weight per row");
    }
    return w;
}

// the levels of the quantile objective (include/gbrl_hip.h, "Quantile regression"): None (empty), a scalar broadcast to the D outputs, or a sequence of D;
// the levels themselves are checked behind the C ABI, which names the output
std::vector<float> read_alpha(const py::object &alpha, int D, const std::string &fn) {
    std::vector<float> a;
    if (alpha.is_none()) return a;
    if (py::isinstance<py::float_>(alpha) || py::isinstance<py::int_>(alpha)) {
        a.assign(static_cast<size_t>(std::max(D, 1)), alpha.cast<float>());
        return a;
    }
    py::array_t<float, py::array::c_style | py::array::forcecast> arr = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(alpha);
    if (!arr) fail(fn + ": alpha must be a number or a sequence of numbers");
    if (arr.ndim() == 0) {
        a.assign(static_cast<size_t>(std::max(D, 1)), *arr.data());
        return a;
    }
    if (arr.ndim() != 1 || arr.shape(0) != D) fail_cat(fn, ": alpha must be a scalar or hold one level per output (", D, ")");
    a.assign(arr.data(), arr.data() + D);
    return a;
}

int read_ndcg_at(py::object &ndcg_at, const std::string &fn) {
    if (ndcg_at.is_none()) return 0;
    const long long k = ndcg_at.cast<long long>();
    if (k < 0 || k > 0x7fffffffLL) fail(fn + ": ndcg_at must be positive (or 0 / None for no truncation), got " + std::to_string(k));
    return static_cast<int>(k);
}
// group: the query sizes, any integer sequence -> int32 (a size that does not fit is refused here, naming the query)
std::vector<int32_t> read_group(py::object &group, const std::string &fn, const char *name) {
    const std::string gname(name);
    if (group.is_none()) fail(fn + ": a ranking objective needs " + gname + ", the sizes of the queries' consecutive row runs");
    py::array_t<int64_t, py::array::c_style | py::array::forcecast> g = py::array_t<int64_t, py::array::c_style | py::array::forcecast>::ensure(group);
    if (!g || g.ndim() != 1) fail(fn + ": " + gname + " must be a one-dimensional sequence of integers");
    std::vector<int32_t> out(static_cast<size_t>(g.size()));
    for (py::ssize_t q = 0; q < g.size(); ++q) {
        const int64_t v = g.data()[q];
        if (v < 1 || v > 0x7fffffffLL) fail(fn + ": " + gname + "[" + std::to_string(q) + "] = " + std::to_string(v) + " (query " + std::to_string(q) + ") is outside [1, 1024]");
        out[static_cast<size_t>(q)] = static_cast<int32_t>(v);
    }
    if (out.empty()) fail(fn + ": a ranking objective needs " + gname + ", the sizes of the queries' consecutive row runs");
    return out;
}
Input read_rank_labels(py::object &labels, const std::string &fn, int n) {
    if (py::isinstance<py::array>(labels) && !py::isinstance<py::array_t<int32_t>>(labels)) fail(fn + ": labels must be an int32 array of shape (n,)");
    Input l = require_input(labels, "labels", fn, 2);
    if (l.shape.size() != 1 || l.shape[0] != static_cast<size_t>(n)) fail(fn + ": labels must be an int32 array of shape (" + std::to_string(n) + ",)");
    return l;
}

int read_n_trees(py::object &n_trees_obj) {   // None: every tree (-1); anything else is checked behind the C ABI
    if (n_trees_obj.is_none()) return -1;
    const long long k = n_trees_obj.cast<long long>();
    return k < INT32_MIN ? INT32_MIN : k > INT32_MAX ? INT32_MAX : static_cast<int>(k);
}

}  // namespace gbrl_py
