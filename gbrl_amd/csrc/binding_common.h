// binding_common.h -- the vocabulary the Python binding (binding.cpp) reads its arguments and delivers its results with.
//
// The shared types live in a named namespace, so that the binding's bodies can be spread over several translation units: pybind11 finds a registered
// class by its typeid, and a type of an anonymous namespace is another type in every unit.  -fvisibility=hidden keeps the names out of the module's
// dynamic symbol table.
#pragma once

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <optional>
#include <sstream>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/gbrl_hip.h"
#include "binding_result.h"

namespace py = pybind11;

namespace gbrl_py {

[[noreturn]] void fail(const std::string &msg);
template <typename... Parts>
[[noreturn]] void fail_cat(const Parts &...parts) {   // a refusal put together from parts, each as a stream writes it
    std::stringstream ss;
    (ss << ... << parts);
    fail(ss.str());
}
// a C ABI status: anything but GBRL_HIP_OK raises the library's last error.  Touches no Python object, so it wraps the call inside a GIL-released block
void check(int status);

// a buffer handed over as a "dltensor" capsule (kDLROCM on the device, kDLCPU on the host), float32 or int32
py::object make_dlpack(void *data, const std::vector<int64_t> &shape, bool on_device, int device_id, bool int32 = false);

struct Input {
    const void *ptr = nullptr;
    std::vector<size_t> shape;
    bool on_device = false;
    py::object keep;  // keeps a converted NumPy array alive for the duration of the call
    const float *f32() const { return static_cast<const float *>(ptr); }
    const int32_t *i32() const { return static_cast<const int32_t *>(ptr); }
    const char *cells() const { return static_cast<const char *>(ptr); }   // 128-byte categorical cells
};

// None | NumPy array | (data_ptr, shape, dtype, device).  `categorical`: 0 = float32 values, 1 = 128-byte cells, 2 = int32
Input read_input(py::object &obj, const std::string &name, bool none_allowed, const std::string &fn, int categorical);
// read_input of an argument the call cannot do without: None and a null pointer get the same "Cannot call <fn> without <name>!"
Input require_input(py::object &obj, const std::string &name, const std::string &fn, int categorical = 0);
// the host rules take NumPy arrays: a device tuple is refused with `text`
void require_host(const Input &in, const std::string &text);

int parse_enum(const std::string &s, std::initializer_list<std::pair<const char *, int>> opts, const char *err);
int parse_device(const std::string &s);
int parse_parity_mode(const std::string &s);
int parse_objective(const std::string &s);
int parse_metric(const std::string &s);
int parse_leaf_update(const std::string &s);
const char *parity_mode_name(int mode);

class PyGBRL {
   public:
    gbrl_hip_model *h = nullptr;
    int device = 0;  // 0 = "cpu" delivery (NumPy), 1 = "cuda" delivery (DLPack / kDLROCM)

    PyGBRL(int input_dim, int output_dim, int policy_dim, int max_depth, int min_data_in_leaf, int n_bins, int par_th,
           float cv_beta, const std::string &split_score_func, const std::string &generator_type, bool use_cv,
           int batch_size, const std::string &grow_policy, int verbose, const std::string &dev, const std::string &name,
           const std::string &parity_mode = "default") {
        gbrl_hip_config c{};
        c.input_dim = input_dim; c.output_dim = output_dim; c.policy_dim = policy_dim; c.max_depth = max_depth;
        c.min_data_in_leaf = min_data_in_leaf; c.n_bins = n_bins; c.par_th = par_th; c.cv_beta = cv_beta;
        // string parsing as types.cpp:31-62
        c.split_score_func = parse_enum(split_score_func, {{"L2", 0}, {"l2", 0}, {"Cosine", 1}, {"cosine", 1}},
                                        "Invalid score function! Options are: Cosine/L2");
        c.generator_type = parse_enum(generator_type, {{"uniform", 0}, {"Uniform", 0}, {"quantile", 1}, {"Quantile", 1}},
                                      "Invalid generator function! Options are: Uniform/Quantile");
        c.grow_policy = parse_enum(grow_policy, {{"greedy", 0}, {"Greedy", 0}, {"oblivious", 1}, {"Oblivious", 1}},
                                   "Invalid generator function! Options are: Greedy/Oblivious");
        c.use_control_variates = use_cv ? 1 : 0;
        c.batch_size = batch_size; c.verbose = verbose; c.device_ordinal = -1; c.learner_name = name.c_str();
        device = parse_device(dev);
        const int parity = parse_parity_mode(parity_mode);
        h = gbrl_hip_create(&c);
        if (!h) fail(gbrl_hip_last_error());
        if (gbrl_hip_set_parity_mode(h, parity, 0) != GBRL_HIP_OK) { gbrl_hip_destroy(h); h = nullptr; fail(gbrl_hip_last_error()); }
    }
    explicit PyGBRL(const PyGBRL &o) : device(o.device) {
        h = gbrl_hip_clone(o.h);
        if (!h) fail(gbrl_hip_last_error());
    }
    explicit PyGBRL(gbrl_hip_model *loaded) : h(loaded), device(0) {}
    ~PyGBRL() { gbrl_hip_destroy(h); }

    gbrl_hip_metadata meta() const {
        gbrl_hip_metadata m{};
        gbrl_hip_get_metadata(h, &m);
        return m;
    }
};

// Extension: a batch binned once and stepped on many times (gbrl_hip_dataset, include/gbrl_hip.h).
class PyDataset {
   public:
    gbrl_hip_dataset *h = nullptr;
    explicit PyDataset(gbrl_hip_dataset *d) : h(d) {}
    PyDataset(const PyDataset &) = delete;
    PyDataset &operator=(const PyDataset &) = delete;
    ~PyDataset() { gbrl_hip_dataset_destroy(h); }
    gbrl_hip_dataset_desc info() const {
        gbrl_hip_dataset_desc d{};
        check(gbrl_hip_dataset_info(h, &d));
        return d;
    }
};

// a ds argument as the C ABI takes it: None is a null handle (the library words the refusal), and its description is all zeros
const gbrl_hip_dataset *dataset_handle(py::object &ds_obj);
gbrl_hip_dataset_desc dataset_info(py::object &ds_obj);

// start_tree_idx / stop_tree_idx: None reads as 0 (stop: "every tree"); what a call refuses about the range is its own
struct TreeRange { int start, stop; };
TreeRange read_tree_range(py::object &start_obj, py::object &stop_obj);

// a one-dimensional obs of `len` values is one row of in_dim features, or a column of `len` rows
void one_dim_obs(size_t len, int in_dim, int &n, int &n_features);

// rows, numeric and categorical feature counts of a predict batch: shape inference for 1-D inputs as binding.cpp:820-923
struct BatchShape { int n, n_num, n_cat; };
BatchShape infer_batch(const Input &o, const Input &c, int in_dim);

// ---- the three blocks every predict-family method is made of
// obs and cat_obs of function `fn` (ids: cat_obs holds int32 dictionary ids, the _encoded methods) and the batch they announce.  A call with a
// base or targets names it as `extra`: it is read between the observations and the shape inference, so that a missing one is reported first.
struct Batch { Input o, c, extra; BatchShape s; };
Batch read_batch(py::object &obs, py::object &cat, const std::string &fn, int in_dim, bool ids = false, py::object *extra = nullptr, const char *extra_name = nullptr);

// `a` (base or targets) is [n, D], or [n] when D == 1
void check_rows_by_outputs(const Input &a, const char *name, int n, int D);

// rows and output dim of step's gradients (`noun` "Gradient") or fit's targets ("Targets"): [n, D], or 1-D -- one row of D > 1 outputs, else n rows
struct OutputRows { int n, dim; };
OutputRows read_output_rows(const Input &a, int output_dim, const char *noun);

// the device a result goes to when it goes to a device: the model's (one rank per GPU: not necessarily device 0)
int result_device(PyGBRL &self, bool on_device);

struct DeviceMem {
    static void *alloc(int device_id, size_t bytes) { return gbrl_hip_device_alloc_on(device_id, bytes); }
    static void free(void *p) { gbrl_hip_device_free(p); }
};

// The result of a call, `count` elements, on a device or new[] on the host.  Freed when the call fails; release() hands it to a DLPack capsule or a
// NumPy array.  adopt() is the in-place form: the caller's own buffer, never freed, and release() returns None.
template <typename T>
class Result : public ResultBuffer<T, DeviceMem> {
    using Buffer = ResultBuffer<T, DeviceMem>;

   public:
    Result(bool on_device, int device_id, size_t count) : Buffer(on_device, device_id, count) {
        if (!this->get()) fail(gbrl_hip_last_error());
    }
    // where the model delivers: its device for "cuda" delivery (the capsule says which), the host otherwise
    Result(PyGBRL &self, size_t count) : Result(self.device == 1, result_device(self, self.device == 1), count) {}
    static Result adopt(const Input &callers) { return Result(callers); }
    py::object release(const std::vector<int64_t> &shape, bool dlpack_on_host = false) {
        if (this->adopted()) return py::none();
        T *p = this->take();
        if (this->on_device() || dlpack_on_host) return make_dlpack(p, shape, this->on_device(), this->device_id(), /*int32=*/std::is_same<T, int32_t>::value);
        py::capsule owner(p, [](void *q) { delete[] static_cast<T *>(q); });
        return py::array_t<T>(std::vector<py::ssize_t>(shape.begin(), shape.end()), p, owner);
    }

   private:
    explicit Result(const Input &callers) : Buffer(typename Buffer::Adopt{}, static_cast<T *>(const_cast<void *>(callers.ptr)), callers.on_device) {}
};
inline std::vector<int64_t> shape_of(const Input &a) { return std::vector<int64_t>(a.shape.begin(), a.shape.end()); }

// ---- argument readers (each refuses in the name of the calling function `fn`)
std::vector<int32_t> read_stops(py::object &stops_obj, int n_trees);   // stops=: strictly ascending tree counts; None: 1 .. n_trees
Input read_rows(py::object &rows, const std::string &fn);              // rows=None | int32 NumPy vector | (data_ptr, (m,), "torch.int32", device)
// A rows= argument as the C ABI takes it: the pointer (None: null, every row), where it lives, and m -- the vector's length, else the data set's
// rows, else those of the call's first array.
struct RowsArg {
    const int32_t *ptr;
    int on_device, m;
};
RowsArg read_rows_arg(py::object &rows, const std::string &fn, py::object &ds_obj, const Input &first);
std::vector<int32_t> read_cols(py::object &cols, const std::string &fn);
Input read_objective_targets(py::object &targets, const char *name, bool none_allowed, const std::string &fn, int objective, int n, int D, bool check_shape);
Input read_weights(py::object &weights, const char *name, const std::string &fn, int n, bool check_shape);
std::vector<float> read_alpha(const py::object &alpha, int D, const std::string &fn);
int read_ndcg_at(py::object &ndcg_at, const std::string &fn);
std::vector<int32_t> read_group(py::object &group, const std::string &fn, const char *name = "group");
Input read_rank_labels(py::object &labels, const std::string &fn, int n);
int read_n_trees(py::object &n_trees_obj);

}  // namespace gbrl_py
