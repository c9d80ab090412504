// binding.cpp -- Python extension module `gbrl_cpp` exposing class `GBRL`, written against include/gbrl_hip.h ONLY.
//
// It mirrors the reference's Python-visible operator interface for the hot path (gbrl/src/cpp/binding.cpp:421-1131):
// same constructor keywords and defaults, same method names, same argument conventions (NumPy arrays or the 4-tuples
// (data_ptr, shape, dtype, device) that gbrl/common/utils.py:43-60 builds from torch tensors), same shape inference for
// 1-D inputs, same RuntimeError conditions, same return conventions (NumPy on "cpu", DLPack capsule on "cuda").
// Differences that are deliberate:
//   * every computation runs on the GPU; `device` only selects how predict() delivers its result.
//   * the DLPack capsule carries kDLROCM (10): torch-ROCm rejects the reference's hard-coded kDLCUDA.
//   * export / SHAP / print are served from the host copy of the ensemble (csrc/explain.cpp); plot_tree raises the
//     reference's own no-Graphviz error (this image has no Graphviz).
#include "binding_common.h"

using namespace gbrl_py;

namespace {

py::object predict_impl(PyGBRL &self, py::object &obs, py::object &cat, py::object start_obj, py::object stop_obj,
                        bool return_torch, const uint64_t *ids_token = nullptr /* non-null: `cat` holds int32 dictionary ids (predict_encoded) */) {
    const gbrl_hip_metadata md = self.meta();
    const auto [start, stop] = read_tree_range(start_obj, stop_obj);
    // bounds as binding.cpp:800-811
    if (start < 0 || (start >= md.n_trees && md.n_trees > 0)) fail_cat("start_tree_idx is out of bounds! Got ", start, ", but valid range is [0, ", md.n_trees - 1, "]");
    if (stop < 0 || stop > md.n_trees) fail_cat("stop_tree_idx is out of bounds! Got ", stop, ", but valid range is [0, ", md.n_trees, "]");
    const Batch b = read_batch(obs, cat, "predict", md.input_dim, ids_token != nullptr);
    const Input &o = b.o, &c = b.c;
    const int n = b.s.n, n_num = b.s.n_num, n_cat = b.s.n_cat;
    const int D = md.output_dim;
    std::vector<int64_t> shape;
    if (D == 1) shape = {n}; else shape = {n, D};  // binding.cpp:281-286
    Result<float> out(self, static_cast<size_t>(n) * D);
    {
        py::gil_scoped_release release;  // binding.cpp:934
        if (ids_token)
            check(gbrl_hip_predict_encoded(self.h, o.f32(), o.on_device, c.i32(), c.on_device, *ids_token, n, n_num, n_cat, start, stop, out.get(), out.on_device()));
        else
            check(gbrl_hip_predict(self.h, o.f32(), o.on_device, c.cells(), c.on_device, n, n_num, n_cat, start, stop, out.get(), out.on_device()));
    }
    return out.release(shape, return_torch);
}

// Extension: predict_continue(obs, categorical_obs, base, start, stop) / predict_continue_encoded(obs, ids, token, base, start, stop): `base`, the
// caller's prediction over the trees [0, start), carried through the trees [start, stop) (include/gbrl_hip.h).  A float32 NumPy `base` of shape
// [n, D] ([n] when D == 1) is left untouched and a new array is returned; a (data_ptr, shape, "torch.float32", device) tuple is updated in place
// and None is returned.
py::object predict_continue_impl(PyGBRL &self, py::object &obs, py::object &cat, py::object &base, py::object start_obj, py::object stop_obj,
                                 const uint64_t *ids_token = nullptr) {
    const gbrl_hip_metadata md = self.meta();
    const auto [start, stop] = read_tree_range(start_obj, stop_obj);
    const Batch batch = read_batch(obs, cat, "predict_continue", md.input_dim, ids_token != nullptr, &base, "base");
    const Input &o = batch.o, &c = batch.c, &b = batch.extra;
    const int n = batch.s.n, n_num = batch.s.n_num, n_cat = batch.s.n_cat, D = md.output_dim;
    check_rows_by_outputs(b, "base", n, D);
    Result<float> out = py::isinstance<py::tuple>(base) ? Result<float>::adopt(b) : Result<float>(false, 0, static_cast<size_t>(n) * D);
    {
        py::gil_scoped_release release;
        if (ids_token)
            check(gbrl_hip_predict_continue_encoded(self.h, o.f32(), o.on_device, c.i32(), c.on_device,
                                                    *ids_token, n, n_num, n_cat, start, stop, b.f32(), b.on_device, out.get(), out.on_device()));
        else
            check(gbrl_hip_predict_continue(self.h, o.f32(), o.on_device, c.cells(), c.on_device, n, n_num,
                                            n_cat, start, stop, b.f32(), b.on_device, out.get(), out.on_device()));
    }
    return out.release(shape_of(b));
}

// Extension: predict_staged(obs, categorical_obs, stops=None) / staged_loss(obs, categorical_obs, targets, stops=None): every ensemble prefix in
// one walk (include/gbrl_hip.h).  `stops`: a strictly ascending sequence of tree counts k, 0 <= k <= n_trees; k == 0 is the bias alone (0 never
// means "all trees" here); None means 1, 2, ..., n_trees.  predict_staged returns float32 [len(stops), n, D] ([len(stops), n] when D == 1) --
// NumPy for a "cpu" model, a DLPack capsule on the model's device for a "cuda" one, as predict does; staged_loss returns float64 [len(stops)].

py::object predict_staged_impl(PyGBRL &self, py::object &obs, py::object &cat, py::object &stops_obj) {
    const gbrl_hip_metadata md = self.meta();
    const Batch b = read_batch(obs, cat, "predict_staged", md.input_dim);
    const Input &o = b.o, &c = b.c;
    const std::vector<int32_t> stops = read_stops(stops_obj, md.n_trees);
    const int n = b.s.n, D = md.output_dim, S = static_cast<int>(stops.size());
    std::vector<int64_t> shape;
    if (D == 1) shape = {S, n}; else shape = {S, n, D};
    Result<float> out(self, static_cast<size_t>(S) * n * D);
    {
        py::gil_scoped_release release;
        check(gbrl_hip_predict_staged(self.h, o.f32(), o.on_device, c.cells(), c.on_device, n, b.s.n_num, b.s.n_cat, stops.data(), S, out.get(), out.on_device()));
    }
    return out.release(shape);
}

py::object staged_loss_impl(PyGBRL &self, py::object &obs, py::object &cat, py::object &targets, py::object &stops_obj) {
    const gbrl_hip_metadata md = self.meta();
    const Batch b = read_batch(obs, cat, "staged_loss", md.input_dim, false, &targets, "targets");
    const Input &o = b.o, &c = b.c, &y = b.extra;
    const BatchShape &bs = b.s;
    const int n = bs.n, D = md.output_dim;
    check_rows_by_outputs(y, "targets", n, D);
    const std::vector<int32_t> stops = read_stops(stops_obj, md.n_trees);
    py::array_t<double> loss(static_cast<py::ssize_t>(stops.size()));
    double *lp = loss.mutable_data();
    {
        py::gil_scoped_release release;
        check(gbrl_hip_staged_loss(self.h, o.f32(), o.on_device, c.cells(), c.on_device,
                                    y.f32(), y.on_device, n, bs.n_num, bs.n_cat, stops.data(), static_cast<int>(stops.size()), lp));
    }
    return loss;
}

// Extension: refit_leaves(obs, categorical_obs, targets, start_tree_idx=0, stop_tree_idx=0, decay_rate=0.0): the leaf values of the trees
// [start, stop) fitted again on this batch, the structure kept (include/gbrl_hip.h).  Returns the MultiRMSE loss of the refitted prefix, a float:
// staged_loss(obs, categorical_obs, targets, stops=[stop])[0] called right after, bit for bit.
double refit_leaves_impl(PyGBRL &self, py::object &obs, py::object &cat, py::object &targets, py::object start_obj, py::object stop_obj, double decay) {
    const gbrl_hip_metadata md = self.meta();
    const auto [start, stop] = read_tree_range(start_obj, stop_obj);
    const Batch b = read_batch(obs, cat, "refit_leaves", md.input_dim, false, &targets, "targets");
    const Input &o = b.o, &c = b.c, &y = b.extra;
    const BatchShape &bs = b.s;
    const int n = bs.n, D = md.output_dim;
    check_rows_by_outputs(y, "targets", n, D);
    double loss = 0.0;
    {
        py::gil_scoped_release release;
        check(gbrl_hip_refit_leaves(self.h, o.f32(), o.on_device, c.cells(), c.on_device, y.f32(), y.on_device, n, bs.n_num, bs.n_cat, start, stop, decay, &loss));
    }
    return loss;
}

// Extension: predict_leaves(obs, categorical_obs, start, stop) / leaf_counts(...) and their _encoded variants (obs, ids, token, start, stop): where
// a row lands (include/gbrl_hip.h).  predict_leaves returns int32 [n, stop - start] global leaf indices -- NumPy for a "cpu" model, a DLPack
// capsule on the model's device for a "cuda" one; leaf_counts returns int64 NumPy [n_leaves], the rows of the batch per global leaf.
py::object leaves_impl(PyGBRL &self, py::object &obs, py::object &cat, py::object start_obj, py::object stop_obj, bool counts,
                       const uint64_t *ids_token = nullptr) {
    const gbrl_hip_metadata md = self.meta();
    const char *fn = counts ? "leaf_counts" : "predict_leaves";
    const auto [start, stop] = read_tree_range(start_obj, stop_obj);
    const Batch b = read_batch(obs, cat, fn, md.input_dim, ids_token != nullptr);
    const Input &o = b.o, &c = b.c;
    const int n = b.s.n, n_num = b.s.n_num, n_cat = b.s.n_cat;
    // the engine checks the same (c_api callers); here too because the result is allocated before the C call
    if (md.n_trees == 0) fail(std::string(fn) + ": the model has no trees");
    const int resolved = stop == 0 ? md.n_trees : stop;
    if (start < 0 || stop < 0 || resolved > md.n_trees || start >= resolved) fail_cat(fn, ": invalid tree range [", start, ", ", stop, ") for ", md.n_trees, " trees");
    if (counts) {
        py::array_t<int64_t> res(static_cast<py::ssize_t>(md.n_leaves));
        int64_t *rp = res.mutable_data();
        {
            py::gil_scoped_release release;
            if (ids_token)
                check(gbrl_hip_leaf_counts_encoded(self.h, o.f32(), o.on_device, c.i32(), c.on_device, *ids_token, n, n_num, n_cat, start, stop, rp));
            else
                check(gbrl_hip_leaf_counts(self.h, o.f32(), o.on_device, c.cells(), c.on_device, n, n_num, n_cat, start, stop, rp));
        }
        return res;
    }
    const int T = resolved - start;
    if (static_cast<int64_t>(n) * T >= (int64_t(1) << 31)) fail("predict_leaves: n_samples x trees >= 2^31 indices: slice the tree range");
    Result<int32_t> out(self, static_cast<size_t>(n) * T);
    {
        py::gil_scoped_release release;
        if (ids_token)
            check(gbrl_hip_predict_leaves_encoded(self.h, o.f32(), o.on_device, c.i32(), c.on_device,
                                                  *ids_token, n, n_num, n_cat, start, stop, out.get(), out.on_device()));
        else
            check(gbrl_hip_predict_leaves(self.h, o.f32(), o.on_device, c.cells(), c.on_device, n, n_num, n_cat, start, stop, out.get(), out.on_device()));
    }
    return out.release({n, T});
}

// Extension: (ids, token) = encode_categorical(categorical_obs): int32 dictionary ids [n, n_cat] of a batch of cells -- a DLPack capsule on the
// model's device for a "cuda" model, a NumPy array otherwise -- for predict_encoded(obs, ids, token, ...).
py::tuple encode_categorical_impl(PyGBRL &self, py::object &cat) {
    Input c = require_input(cat, "cat_obs", "encode_categorical", 1);
    const int n = static_cast<int>(c.shape[0]), n_cat = c.shape.size() > 1 ? static_cast<int>(c.shape[1]) : 1;
    Result<int32_t> ids(self, static_cast<size_t>(n) * n_cat);
    uint64_t token = 0;
    {
        py::gil_scoped_release release;
        check(gbrl_hip_encode_categorical(self.h, c.cells(), c.on_device, n, n_cat, ids.get(), ids.on_device(), &token));
    }
    return py::make_tuple(ids.release({n, n_cat}), token);
}

// What step and fit read alike (binding.cpp:462-515, 541-556): the gradients or targets (`first`, called `noun` where their output dim is refused)
// give n and the output dim; obs and cat_obs are then held against n -- a 1-D one is one row when n == 1, else a column -- and the feature total
// against input_dim.  fit words its row-count refusals as step does ("gradient samples").
struct SampleShape { Input first, o, c; int n = 0, n_num = 0, n_cat = 0; };
SampleShape read_sample_shape(const gbrl_hip_metadata &md, const std::string &fn, py::object &first, const char *first_name, const char *noun, py::object &obs,
                              py::object &cat) {
    SampleShape s;
    s.first = read_input(first, first_name, false, fn, false);
    s.n = read_output_rows(s.first, md.output_dim, noun).n;
    auto rows_and_width = [&](const Input &a, int &width, const char *what) {
        if (!a.ptr) return;
        int rows;
        if (a.shape.size() == 1) { width = (s.n == 1) ? static_cast<int>(a.shape[0]) : 1; rows = (s.n == 1) ? 1 : static_cast<int>(a.shape[0]); }
        else { rows = static_cast<int>(a.shape[0]); width = static_cast<int>(a.shape[1]); }
        if (rows != s.n) fail_cat("Number of ", what, " ", rows, " != number of gradient samples ", s.n);
    };
    s.o = read_input(obs, "obs", true, fn, false);
    rows_and_width(s.o, s.n_num, "observations");
    s.c = read_input(cat, "cat_obs", true, fn, true);
    rows_and_width(s.c, s.n_cat, "categorical observations");
    if (s.n_cat + s.n_num != md.input_dim) fail_cat("Total number of features ", s.n_cat + s.n_num, " != correct input dim ", md.input_dim);
    return s;
}

void step_impl(PyGBRL &self, py::object &obs, py::object &cat, py::object &grads) {
    const SampleShape s = read_sample_shape(self.meta(), "step", grads, "grads", "Gradient", obs, cat);
    {
        py::gil_scoped_release release;  // binding.cpp:525
        check(gbrl_hip_step(self.h, s.o.f32(), s.o.on_device, s.c.cells(), s.c.on_device, s.first.f32(), s.first.on_device, s.n, s.n_num, s.n_cat));
    }
}

std::unique_ptr<PyDataset> prepare_dataset_impl(PyGBRL &self, py::object &obs, py::object reference = py::none()) {
    // categorical cells cannot be prepared: their split candidates depend on the step's gradients
    bool cells = false;
    if (py::isinstance<py::array>(obs)) cells = py::array(obs).dtype().kind() == 'S';
    else if (py::isinstance<py::tuple>(obs) && py::len(obs) == 4) { const std::string dt = py::str(obs.cast<py::tuple>()[2]); cells = dt == "S128" || dt == "|S128"; }
    if (cells) fail("prepare_dataset: categorical columns are not supported (their split candidates depend on the step's gradients)");
    const gbrl_hip_metadata md = self.meta();
    Input o = require_input(obs, "obs", "prepare_dataset");
    int n, n_num;
    if (o.shape.size() == 1) one_dim_obs(o.shape[0], md.input_dim, n, n_num);   // as predict reads a 1-D input
    else if (o.shape.size() == 2) { n = static_cast<int>(o.shape[0]); n_num = static_cast<int>(o.shape[1]); }
    else fail("obs must have one or two dimensions");
    gbrl_hip_dataset *d = nullptr;
    if (!reference.is_none()) {   // bound to the reference's thresholds: the width is the reference's
        const PyDataset &ref = reference.cast<const PyDataset &>();
        gbrl_hip_dataset_desc rd{};
        if (gbrl_hip_dataset_info(ref.h, &rd) == GBRL_HIP_OK && n_num != rd.n_features) {
            fail_cat("prepare_dataset: obs has ", n_num, " features, the reference ", rd.n_features);
        }
        {
            py::gil_scoped_release release;
            d = gbrl_hip_dataset_create_like(self.h, ref.h, o.f32(), o.on_device, n);
        }
    } else {
        py::gil_scoped_release release;
        d = gbrl_hip_dataset_create(self.h, o.f32(), o.on_device, n, n_num);
    }
    if (!d) fail(gbrl_hip_last_error());
    return std::unique_ptr<PyDataset>(new PyDataset(d));
}

void step_prepared_impl(PyGBRL &self, py::object ds_obj, py::object &grads, py::object &rows, py::object cols = py::none()) {
    const gbrl_hip_metadata md = self.meta();
    const gbrl_hip_dataset *ds = dataset_handle(ds_obj);
    Input g = read_input(grads, "grads", false, "step_prepared", false);
    const int n = read_output_rows(g, md.output_dim, "Gradient").n;   // as step reads its gradients
    const RowsArg r = read_rows_arg(rows, "step_prepared", ds_obj, g);
    if (!rows.is_none() && r.m != n) fail_cat("Number of rows ", r.m, " != number of gradient samples ", n);
    std::vector<int32_t> cv;
    if (!cols.is_none()) cv = read_cols(cols, "step_prepared");
    static const int32_t kNoCols = 0;   // an empty cols vector is "no column", not "every column"
    {
        py::gil_scoped_release release;
        if (cols.is_none()) check(gbrl_hip_step_prepared(self.h, ds, g.f32(), g.on_device, r.ptr, r.on_device, n));
        else check(gbrl_hip_step_prepared_cols(self.h, ds, g.f32(), g.on_device, r.ptr, r.on_device, n,
                                               cv.empty() ? &kNoCols : cv.data(), static_cast<int>(cv.size())));
    }
}

py::array dataset_codes_impl(PyDataset &self, py::object &rows, py::object &cols) {
    const gbrl_hip_dataset_desc d = self.info();
    Input r = read_rows(rows, "codes");
    const int m = rows.is_none() ? d.n_rows : static_cast<int>(r.shape[0]);
    if (m <= 0) fail("dataset_codes: no rows (m must be positive)");
    std::vector<int32_t> cv;
    if (!cols.is_none()) {
        cv = read_cols(cols, "codes");
        if (cv.empty()) fail("dataset_codes: cols must name between 1 and " + std::to_string(d.n_features) + " columns, got 0");
    }
    const py::ssize_t groups = cols.is_none() ? d.code_groups : static_cast<py::ssize_t>((cv.size() + 15) / 16);
    py::array_t<uint16_t> out({groups, static_cast<py::ssize_t>(m), static_cast<py::ssize_t>(16)});
    uint16_t *op = out.mutable_data();
    {
        py::gil_scoped_release release;
        if (cols.is_none()) check(gbrl_hip_dataset_codes(self.h, r.i32(), r.on_device, m, op));
        else check(gbrl_hip_dataset_codes_cols(self.h, r.i32(), r.on_device, m, cv.data(), static_cast<int>(cv.size()), op));
    }
    return std::move(out);
}

// Extension: the column rule (include/gbrl_hip.h, "Column subsampling"), host only
py::array_t<int32_t> sample_cols_host_impl(int F, double colsample, uint64_t seed, int draw) {
    std::vector<int32_t> cols(static_cast<size_t>(std::max(F, 0)));
    int32_t none = 0;
    int k = 0;
    check(gbrl_hip_sample_cols_host(F, colsample, seed, draw, cols.empty() ? &none : cols.data(), &k));
    py::array_t<int32_t> out(static_cast<py::ssize_t>(k));
    std::copy(cols.begin(), cols.begin() + k, out.mutable_data());
    return out;
}

// Extension: the row sampler (include/gbrl_hip.h, "Row subsampling").  PreparedDataset.sample_rows -> int32 [m] on the data set's device, handed
// out as predict hands out device results (a DLPack capsule; the buffer holds stop - start entries, of which the first m are the tensor).
py::object dataset_sample_rows_impl(PyDataset &self, double subsample, uint64_t seed, int draw, int start, py::object stop_obj) {
    const gbrl_hip_dataset_desc d = self.info();
    const int stop = stop_obj.is_none() ? d.n_rows : stop_obj.cast<int>();
    if (start < 0 || stop > d.n_rows || stop <= start) fail_cat("sample_rows: rows [", start, ", ", stop, ") are not a non-empty range inside [0, ", d.n_rows, ")");
    const int n = stop - start;
    Result<int32_t> out(true, d.device, static_cast<size_t>(n));
    int m = 0;
    {
        py::gil_scoped_release release;
        check(gbrl_hip_dataset_sample_rows(self.h, start, n, subsample, seed, draw, out.get(), 1, &m));
    }
    return out.release({static_cast<int64_t>(m)});
}

py::array_t<int32_t> sample_rows_host_impl(int n, double subsample, uint64_t seed, int draw, int row0) {
    std::vector<int32_t> rows(static_cast<size_t>(std::max(n, 0)));
    int32_t none = 0;
    int m = 0;
    check(gbrl_hip_sample_rows_host(row0, n, subsample, seed, draw, rows.empty() ? &none : rows.data(), &m));
    py::array_t<int32_t> out(static_cast<py::ssize_t>(m));
    std::copy(rows.begin(), rows.begin() + m, out.mutable_data());
    return out;
}

// Extension: one-side sampling (include/gbrl_hip.h, "One-side sampling").  The gradient rows of a range: float32 [n, D] or [n] (D = 1).
struct GossGrads { Input g; int n = 0, D = 1; bool flat = false; };
GossGrads read_goss_grads(py::object &grads, const std::string &fn) {
    GossGrads r;
    r.g = require_input(grads, "grads", fn);
    if (r.g.shape.empty() || r.g.shape.size() > 2) fail("grads must be a float32 array of shape (n, D) or (n,)");
    r.flat = r.g.shape.size() == 1;
    r.n = static_cast<int>(r.g.shape[0]);
    r.D = r.flat ? 1 : static_cast<int>(r.g.shape[1]);
    return r;
}

// gbrl_cpp.goss_rows_host(grads, top_rate, other_rate, seed=0, draw=0, row0=0) -> (rows int32 [m], factor float32 [m])
py::tuple goss_rows_host_impl(py::object &grads, double top_rate, double other_rate, uint64_t seed, int draw, int row0) {
    GossGrads in = read_goss_grads(grads, "goss_rows_host");
    require_host(in.g, "goss_rows_host takes a NumPy array");
    std::vector<int32_t> rows(static_cast<size_t>(std::max(in.n, 1)));
    std::vector<float> factor(rows.size());
    int m = 0;
    check(gbrl_hip_goss_rows_host(in.g.f32(), in.D, row0, in.n, top_rate, other_rate, seed, draw, rows.data(), factor.data(), nullptr, &m));
    py::array_t<int32_t> ro(static_cast<py::ssize_t>(m));
    py::array_t<float> fo(static_cast<py::ssize_t>(m));
    std::copy(rows.begin(), rows.begin() + m, ro.mutable_data());
    std::copy(factor.begin(), factor.begin() + m, fo.mutable_data());
    return py::make_tuple(ro, fo);
}

// PreparedDataset.sample_goss(grads, top_rate, other_rate, seed=0, draw=0, start=0, stop=None) -> {'rows', 'factor', 'grads', 'n_top', 'tau_bits'}:
// NumPy arrays for a NumPy grads, DLPack capsules on the data set's device for a device tuple (each buffer holds stop - start rows, of which the
// first m are the tensor), as sample_rows hands its rows out.
py::dict dataset_sample_goss_impl(PyDataset &self, py::object &grads, double top_rate, double other_rate, uint64_t seed, int draw, int start, py::object stop_obj) {
    const gbrl_hip_dataset_desc d = self.info();
    const int stop = stop_obj.is_none() ? d.n_rows : stop_obj.cast<int>();
    if (start < 0 || stop > d.n_rows || stop <= start) fail_cat("sample_goss: rows [", start, ", ", stop, ") are not a non-empty range inside [0, ", d.n_rows, ")");
    const int n = stop - start;
    GossGrads in = read_goss_grads(grads, "sample_goss");
    if (in.n != n) fail_cat("sample_goss: grads has ", in.n, " rows, the range [", start, ", ", stop, ") has ", n);
    const size_t n_el = static_cast<size_t>(n) * static_cast<size_t>(std::max(in.D, 1));
    const bool dev = in.g.on_device;
    // device results hold the whole range and are handed out as they are; host results are written to vectors and their first m entries copied out
    std::optional<Result<int32_t>> drows;
    std::optional<Result<float>> dfactor, dgrads;
    std::vector<int32_t> hrows;
    std::vector<float> hfactor, hgrads;
    if (dev) {
        drows.emplace(true, d.device, static_cast<size_t>(n)); dfactor.emplace(true, d.device, static_cast<size_t>(n)); dgrads.emplace(true, d.device, n_el);
    } else {
        hrows.resize(static_cast<size_t>(n)); hfactor.resize(static_cast<size_t>(n)); hgrads.resize(n_el);
    }
    int32_t *rp = dev ? drows->get() : hrows.data();
    float *fp = dev ? dfactor->get() : hfactor.data(), *gp = dev ? dgrads->get() : hgrads.data();
    int m = 0, n_top = 0;
    uint32_t tau = 0;
    {
        py::gil_scoped_release release;
        check(gbrl_hip_dataset_sample_goss(self.h, in.g.f32(), in.D, start, n, top_rate, other_rate, seed, draw, rp, fp, gp, dev ? 1 : 0, &m, &n_top, &tau));
    }
    py::dict out;
    std::vector<int64_t> gshape{static_cast<int64_t>(m)};
    if (!in.flat) gshape.push_back(in.D);
    if (dev) {
        out["rows"] = drows->release({static_cast<int64_t>(m)});
        out["factor"] = dfactor->release({static_cast<int64_t>(m)});
        out["grads"] = dgrads->release(gshape);
    } else {
        py::array_t<int32_t> ro(static_cast<py::ssize_t>(m));
        py::array_t<float> fo(static_cast<py::ssize_t>(m));
        py::array_t<float> go(std::vector<py::ssize_t>(gshape.begin(), gshape.end()));
        std::copy(hrows.begin(), hrows.begin() + m, ro.mutable_data());
        std::copy(hfactor.begin(), hfactor.begin() + m, fo.mutable_data());
        std::copy(hgrads.begin(), hgrads.begin() + static_cast<size_t>(m) * in.D, go.mutable_data());
        out["rows"] = ro; out["factor"] = fo; out["grads"] = go;
    }
    out["n_top"] = py::int_(n_top);
    out["tau_bits"] = py::int_(tau);
    return out;
}

// Extension: the walk over a data set's bin codes (include/gbrl_hip.h).  condition_bins(thresholds) -> int32 array shaped like feature_values.
py::array_t<int32_t> condition_bins_impl(PyGBRL &self, py::object &thresholds) {
    const gbrl_hip_metadata md = self.meta();
    Input t = read_input(thresholds, "thresholds", false, "condition_bins", false);
    require_host(t, "condition_bins takes a NumPy array");
    if (t.shape.size() != 2) fail("thresholds must be a float32 array of shape (n_features, n_bins)");
    const py::ssize_t S = md.grow_policy == GBRL_HIP_GROW_OBLIVIOUS ? md.n_trees : md.n_leaves;
    py::array_t<int32_t> out({S, static_cast<py::ssize_t>(md.max_depth)});
    check(gbrl_hip_condition_bins(self.h, t.f32(), static_cast<int>(t.shape[0]), static_cast<int>(t.shape[1]), out.mutable_data()));
    return out;
}

// predict_continue_prepared(ds, base, start, stop, rows=None): predict_continue's conventions for base and the range, step_prepared's for rows
py::object predict_continue_prepared_impl(PyGBRL &self, py::object ds_obj, py::object &base, py::object start_obj, py::object stop_obj, py::object &rows) {
    const gbrl_hip_metadata md = self.meta();
    const gbrl_hip_dataset *ds = dataset_handle(ds_obj);
    const auto [start, stop] = read_tree_range(start_obj, stop_obj);
    Input b = require_input(base, "base", "predict_continue_prepared");
    const RowsArg r = read_rows_arg(rows, "predict_continue_prepared", ds_obj, b);
    const int D = md.output_dim, m = r.m;
    check_rows_by_outputs(b, "base", m, D);
    Result<float> out = py::isinstance<py::tuple>(base) ? Result<float>::adopt(b) : Result<float>(false, 0, std::max<size_t>(static_cast<size_t>(m) * D, 1));
    {
        py::gil_scoped_release release;
        check(gbrl_hip_predict_continue_prepared(self.h, ds, r.ptr, r.on_device, m, b.f32(), b.on_device, start, stop, out.get()));
    }
    return out.release(shape_of(b));
}

// fit_prepared(ds, targets, iterations, valid=None, valid_targets=None, early_stopping_rounds=0, min_delta=0.0, subsample=1.0, colsample=1.0, seed=0,
// objective='rmse', eval_metric=None, leaf_update='gradient', leaf_l2=1.0, weights=None, valid_weights=None): a float without a validation set (the three validation arguments at their defaults), else a dict; the other keywords go
// with either.  A missing valid_targets is left to the C ABI's message.
py::object fit_prepared_impl(PyGBRL &self, py::object ds_obj, py::object &targets, int iterations, py::object valid_obj, py::object &valid_targets,
                             int early_stopping_rounds, double min_delta, double subsample, double colsample, uint64_t seed, const std::string &objective_name,
                             py::object metric_obj, const std::string &leaf_update_name, double leaf_l2, py::object &weights, py::object &valid_weights,
                             py::object goss_obj, py::object alpha_obj, py::object group_obj, py::object ndcg_at_obj, py::object valid_group_obj) {
    const gbrl_hip_metadata md = self.meta();
    // the ranking keywords (include/gbrl_hip.h, "Ranking objectives"): None stays NULL, so that a group with another objective is refused behind the C ABI
    std::vector<int32_t> group, valid_group;
    if (!group_obj.is_none()) group = read_group(group_obj, "fit_prepared");
    if (!valid_group_obj.is_none()) valid_group = read_group(valid_group_obj, "fit_prepared", "valid_group");
    const int ndcg_at = read_ndcg_at(ndcg_at_obj, "fit_prepared");
    const std::vector<float> alpha = read_alpha(alpha_obj, md.output_dim, "fit_prepared");
    double goss_top = 0.0, goss_other = 0.0;
    if (!goss_obj.is_none()) {   // goss=(top_rate, other_rate); an other_rate of 0 is refused here, since 0 means "off" below
        py::sequence g = py::isinstance<py::sequence>(goss_obj) ? goss_obj.cast<py::sequence>() : py::sequence();
        if (!py::isinstance<py::sequence>(goss_obj) || g.size() != 2) fail("fit_prepared: goss must be None or a pair (top_rate, other_rate)");
        goss_top = g[0].cast<double>();
        goss_other = g[1].cast<double>();
        if (goss_other == 0.0) fail("fit_prepared: goss needs other_rate in (0, 1], got 0");
    }
    const gbrl_hip_dataset *ds = dataset_handle(ds_obj);
    const int objective = parse_objective(objective_name), leaf_update = parse_leaf_update(leaf_update_name);
    const int metric = metric_obj.is_none() ? GBRL_HIP_METRIC_NONE : parse_metric(metric_obj.cast<std::string>());
    if (valid_obj.is_none() && (!valid_targets.is_none() || early_stopping_rounds != 0 || min_delta != 0.0))
        fail("fit_prepared: valid_targets, early_stopping_rounds and min_delta need a validation set (valid=)");
    if (valid_obj.is_none() && !valid_weights.is_none()) fail("fit_prepared: valid_weights need a validation set (valid=)");
    if (valid_obj.is_none() && !valid_group_obj.is_none()) fail("fit_prepared: valid_group needs a validation set (valid=)");
    const gbrl_hip_dataset *dsv = dataset_handle(valid_obj);
    const int n = dataset_info(ds_obj).n_rows, nv = dataset_info(valid_obj).n_rows;
    Input w = read_weights(weights, "weights", "fit_prepared", n, ds != nullptr), wv;
    if (dsv) wv = read_weights(valid_weights, "valid_weights", "fit_prepared", nv, true);
    Input t = read_objective_targets(targets, "targets", false, "fit", objective, n, md.output_dim, ds != nullptr);
    Input tv;
    if (dsv) tv = read_objective_targets(valid_targets, "valid_targets", true, "fit", objective, nv, md.output_dim, true);
    std::vector<double> curve(static_cast<size_t>(std::max(iterations, 0)) + 1, 0.0), mcurve(metric != GBRL_HIP_METRIC_NONE ? curve.size() : 0, 0.0);
    float loss = 0.0f, weight_max = 0.0f;
    int done = 0, best = 0;
    {
        py::gil_scoped_release release;
        check(gbrl_hip_fit_prepared_rank(self.h, ds, t.ptr, t.on_device, iterations, dsv, tv.ptr, tv.on_device, early_stopping_rounds, min_delta, subsample,
                                         colsample, seed, objective, metric, leaf_update, leaf_l2, w.f32(), w.on_device, wv.f32(), wv.on_device, goss_top, goss_other,
                                         alpha.empty() ? nullptr : alpha.data(), group.empty() ? nullptr : group.data(), static_cast<int>(group.size()), ndcg_at,
                                         valid_group.empty() ? nullptr : valid_group.data(), static_cast<int>(valid_group.size()), &loss,
                                         dsv ? curve.data() : nullptr, dsv && metric != GBRL_HIP_METRIC_NONE ? mcurve.data() : nullptr, &done, &best, &weight_max));
    }
    if (!dsv) return py::float_(loss);
    py::array_t<double> vl(static_cast<py::ssize_t>(done) + 1);
    std::copy(curve.begin(), curve.begin() + done + 1, vl.mutable_data());
    py::dict out;
    out["loss"] = py::float_(loss);
    out["valid_loss"] = vl;
    out["iterations"] = py::int_(done);
    out["best_n_trees"] = py::int_(best);
    if (metric != GBRL_HIP_METRIC_NONE) {
        py::array_t<double> vm(static_cast<py::ssize_t>(done) + 1);
        std::copy(mcurve.begin(), mcurve.begin() + done + 1, vm.mutable_data());
        out["valid_metric"] = vm;
        out["eval_metric"] = metric_obj;
    }
    if (w.ptr) out["weight_max"] = py::float_(weight_max);
    return std::move(out);
}

// the leaves of a tree (-1: the last).  An index outside the model is left to the C ABI's message: one leaf's room is enough for a call that is refused
py::ssize_t tree_leaf_count(PyGBRL &self, const gbrl_hip_metadata &md, int tree) {
    const py::ssize_t T = md.n_trees;
    if (tree < -1 || tree >= T || T == 0) return 1;
    std::vector<int32_t> ti(static_cast<size_t>(T));
    const py::ssize_t tt = tree == -1 ? T - 1 : tree;
    check(gbrl_hip_get_ensemble(self.h, ti.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    return (tt + 1 < T ? ti[tt + 1] : md.n_leaves) - ti[tt];
}

// the results of the leaves calls: room for `leaves` leaves of D outputs, call(...) -> the C ABI's status, the dict
template <typename Call>
py::dict newton_leaves_result(py::ssize_t leaves, py::ssize_t D, Call &&call) {
    py::array_t<int64_t> sums({leaves, 2 * D + 1});
    py::array_t<float> values({leaves, D});
    int bits = 0;
    check(call(sums.mutable_data(), &bits, values.mutable_data()));
    py::dict out;
    out["sums"] = sums;
    out["bits"] = py::int_(bits);
    out["values"] = values;
    return out;
}
template <typename Call>
py::dict leaf_quantile_result(py::ssize_t leaves, py::ssize_t D, Call &&call) {
    py::array_t<float> values({leaves, D});
    py::array_t<int64_t> counts(std::vector<py::ssize_t>{leaves}), ranks({leaves, D});
    check(call(values.mutable_data(), counts.mutable_data(), ranks.mutable_data()));
    py::dict out;
    out["values"] = values;
    out["counts"] = counts;
    out["ranks"] = ranks;
    return out;
}

// Extension: Newton leaf values (include/gbrl_hip.h, "Newton leaf values").
// newton_leaves_prepared(ds, pred, targets, objective, leaf_l2=1.0, rows=None, tree=-1, weights=None, weight_max=None) -> {'sums': int64 [leaves, 2 D + 1], 'bits', 'values': float32 [leaves, D]}
py::dict newton_leaves_prepared_impl(PyGBRL &self, py::object ds_obj, py::object &pred, py::object &targets, const std::string &objective_name, double leaf_l2,
                                     py::object &rows, int tree, py::object &weights, py::object weight_max_obj, py::object group_obj, py::object ndcg_at_obj) {
    const gbrl_hip_metadata md = self.meta();
    const gbrl_hip_dataset *ds = dataset_handle(ds_obj);
    const int objective = parse_objective(objective_name), D = md.output_dim;
    const bool ranking = objective == GBRL_HIP_OBJ_PAIRWISE || objective == GBRL_HIP_OBJ_LAMBDARANK;
    if (!ranking && (!group_obj.is_none() || !ndcg_at_obj.is_none())) fail("newton_leaves_prepared: group and ndcg_at belong to the ranking objectives 'pairwise' and 'lambdarank'");
    if (ranking) {   // g and h of rank_gradient over every row of the data set, summed from their buffers
        const std::string fn = "newton_leaves_prepared";
        if (!rows.is_none()) fail("newton_leaves_prepared: rows with a ranking objective is not supported (a row list cuts queries apart)");
        if (!weights.is_none() || !weight_max_obj.is_none()) fail("newton_leaves_prepared: weights with a ranking objective are not supported");
        const std::vector<int32_t> grp = read_group(group_obj, fn);
        const int ndcg_at = read_ndcg_at(ndcg_at_obj, fn);
        Input p = require_input(pred, "pred", fn);
        const int n = ds ? dataset_info(ds_obj).n_rows : (p.shape.empty() ? 0 : static_cast<int>(p.shape[0]));
        check_rows_by_outputs(p, "pred", n, 1);
        Input l = read_objective_targets(targets, "targets", false, fn, objective, n, 1, true);
        if (!l.ptr) fail("Cannot call newton_leaves_prepared without targets!");
        return newton_leaves_result(tree_leaf_count(self, md, tree), 1, [&](int64_t *sp, int *bits, float *vp) {
            py::gil_scoped_release release;
            return gbrl_hip_newton_leaves_prepared_rank(self.h, ds, p.f32(), p.on_device, l.i32(), l.on_device,
                                                        grp.data(), static_cast<int>(grp.size()), objective, ndcg_at, tree, leaf_l2, sp, bits, vp);
        });
    }
    Input p = require_input(pred, "pred", "newton_leaves_prepared");
    const RowsArg r = read_rows_arg(rows, "newton_leaves_prepared", ds_obj, p);
    const int m = r.m;
    check_rows_by_outputs(p, "pred", m, D);
    Input t = read_objective_targets(targets, "targets", false, "newton_leaves_prepared", objective, m, D, true);
    if (!t.ptr) fail("Cannot call newton_leaves_prepared without targets!");
    Input w = read_weights(weights, "weights", "newton_leaves_prepared", m, true);
    if (!w.ptr && !weight_max_obj.is_none()) fail("newton_leaves_prepared: weight_max needs weights");
    const float weight_max = weight_max_obj.is_none() ? -1.0f : weight_max_obj.cast<float>();
    if (!weight_max_obj.is_none() && !(weight_max >= 0.0f)) fail("newton_leaves_prepared: weight_max must be in [0, 65536] (and not NaN)");
    return newton_leaves_result(tree_leaf_count(self, md, tree), D, [&](int64_t *sp, int *bits, float *vp) {
        py::gil_scoped_release release;
        return gbrl_hip_newton_leaves_prepared_weighted(self.h, ds, r.ptr, r.on_device, m, p.f32(), p.on_device, t.ptr, t.on_device,
                                                        objective, tree, leaf_l2, w.f32(), w.on_device, weight_max, sp, bits, vp);
    });
}

// Extension: quantile regression (include/gbrl_hip.h, "Quantile regression").
// quantile_leaves_prepared(ds, pred, targets, alpha, rows=None, tree=-1) -> {'values': float32 [leaves, D], 'counts': int64 [leaves], 'ranks': int64 [leaves, D]}
py::dict quantile_leaves_prepared_impl(PyGBRL &self, py::object ds_obj, py::object &pred, py::object &targets, py::object alpha_obj, py::object &rows, int tree) {
    const gbrl_hip_metadata md = self.meta();
    const gbrl_hip_dataset *ds = dataset_handle(ds_obj);
    const int D = md.output_dim;
    const std::vector<float> alpha = read_alpha(alpha_obj, D, "quantile_leaves_prepared");
    Input p = require_input(pred, "pred", "quantile_leaves_prepared");
    const RowsArg r = read_rows_arg(rows, "quantile_leaves_prepared", ds_obj, p);
    const int m = r.m;
    check_rows_by_outputs(p, "pred", m, D);
    Input t = read_objective_targets(targets, "targets", false, "quantile_leaves_prepared", GBRL_HIP_OBJ_QUANTILE, m, D, true);
    if (!t.ptr) fail("Cannot call quantile_leaves_prepared without targets!");
    return leaf_quantile_result(tree_leaf_count(self, md, tree), D, [&](float *vp, int64_t *cp, int64_t *kp) {
        py::gil_scoped_release release;
        return gbrl_hip_quantile_leaves_prepared(self.h, ds, r.ptr, r.on_device, m, p.f32(), p.on_device,
                                                 t.f32(), t.on_device, alpha.empty() ? nullptr : alpha.data(), tree, vp, cp, kp);
    });
}

// the rule on the host: x float32 [m, D] (or [m]), leaves int32 [m] -> {'values', 'counts', 'ranks'}
py::dict leaf_quantile_host_impl(py::array_t<float, py::array::c_style | py::array::forcecast> x, py::array_t<int32_t, py::array::c_style | py::array::forcecast> leaves,
                                 int n_leaves, py::object alpha_obj) {
    if (x.ndim() < 1 || x.ndim() > 2 || leaves.ndim() != 1 || leaves.shape(0) != x.shape(0)) fail("leaf_quantile_host: x float32 [m, D] (or [m]), leaves int32 [m]");
    const py::ssize_t m = x.shape(0), D = x.ndim() == 2 ? x.shape(1) : 1, L = std::max(n_leaves, 1);
    const std::vector<float> alpha = read_alpha(alpha_obj, static_cast<int>(D), "leaf_quantile_host");
    return leaf_quantile_result(L, D, [&](float *vp, int64_t *cp, int64_t *kp) {
        return gbrl_hip_leaf_quantile_host(x.data(), leaves.data(), static_cast<int>(m), static_cast<int>(D), n_leaves, alpha.empty() ? nullptr : alpha.data(), vp, cp, kp);
    });
}

// the hessian rule on the host: no device, no model (the targets do not enter: accepted and ignored, so that the call reads like the gradient's)
py::array_t<float> objective_hessian_host_impl(py::object &pred, py::object targets, const std::string &objective_name, py::object &weights) {
    const int objective = parse_objective(objective_name);
    Input p = read_input(pred, "pred", false, "objective_hessian_host", false);
    require_host(p, "objective_hessian_host takes NumPy arrays");
    if (p.shape.empty() || p.shape.size() > 2) fail("pred must be a float32 array of shape (n, D) or (n,)");
    const int n = static_cast<int>(p.shape[0]), D = p.shape.size() == 2 ? static_cast<int>(p.shape[1]) : 1;
    Input w = read_weights(weights, "weights", "objective_hessian_host", n, true);
    require_host(w, "objective_hessian_host takes NumPy arrays");
    py::array_t<float> out(std::vector<py::ssize_t>(p.shape.begin(), p.shape.end()));
    float none = 0.0f;
    check(gbrl_hip_objective_hessian_host_weighted(p.f32(), w.f32(), n, D, objective, out.size() ? out.mutable_data() : &none));
    return out;
}

// the value rule on the host: sums int64 [leaves, 2 D + 1], old_values float32 [leaves, D], depths int32 [leaves] -> float32 [leaves, D]
py::array_t<float> newton_values_host_impl(py::array_t<int64_t, py::array::c_style | py::array::forcecast> sums, int bits,
                                           py::array_t<float, py::array::c_style | py::array::forcecast> old_values,
                                           py::array_t<int32_t, py::array::c_style | py::array::forcecast> depths, double leaf_l2) {
    if (old_values.ndim() != 2 || sums.ndim() != 2 || depths.ndim() != 1) fail("newton_values_host: sums [leaves, 2 D + 1], old_values [leaves, D], depths [leaves]");
    const py::ssize_t L = old_values.shape(0), D = old_values.shape(1);
    if (sums.shape(0) != L || sums.shape(1) != 2 * D + 1 || depths.shape(0) != L) fail("newton_values_host: sums [leaves, 2 D + 1], old_values [leaves, D], depths [leaves]");
    py::array_t<float> out({L, D});
    check(gbrl_hip_newton_values_host(sums.data(), static_cast<int>(L), static_cast<int>(D), bits, old_values.data(), depths.data(), leaf_l2, out.mutable_data()));
    return out;
}

// the counts of a metric as int64: [D, 3] = (2U_d, P_d, N_d) for auc, [D] (softmax: [1]) for error
py::array_t<int64_t> metric_counts_array(int objective, int metric, int D) {
    const py::ssize_t C = objective == GBRL_HIP_OBJ_SOFTMAX ? 1 : D;
    if (metric == GBRL_HIP_METRIC_AUC) return py::array_t<int64_t>(std::vector<py::ssize_t>{C, 3});
    return py::array_t<int64_t>(std::vector<py::ssize_t>{C});
}

// eval_metric(pred, targets, objective, metric) -> (value, counts): NumPy arrays or device tuples in, a float and an int64 NumPy array out
py::tuple eval_metric_impl(PyGBRL &self, py::object &pred, py::object &targets, const std::string &objective_name, const std::string &metric_name) {
    const gbrl_hip_metadata md = self.meta();
    const int objective = parse_objective(objective_name), metric = parse_metric(metric_name), D = md.output_dim;
    Input p = require_input(pred, "pred", "eval_metric");
    const int n = p.shape.empty() ? 0 : static_cast<int>(p.shape[0]);
    check_rows_by_outputs(p, "pred", n, D);
    Input t = read_objective_targets(targets, "targets", false, "eval_metric", objective, n, D, true);
    if (!t.ptr) fail("Cannot call eval_metric without targets!");
    py::array_t<int64_t> counts = metric_counts_array(objective, metric, D);
    double value = 0.0;
    {
        py::gil_scoped_release release;
        check(gbrl_hip_eval_metric(self.h, p.f32(), p.on_device, t.ptr, t.on_device, n, objective, metric, &value, counts.mutable_data()));
    }
    return py::make_tuple(py::float_(value), counts);
}

// the definitions on the host (include/gbrl_hip.h, "Classifier metrics"): no device, no model
py::tuple eval_metric_host_impl(py::object &pred, py::object &targets, const std::string &objective_name, const std::string &metric_name) {
    const int objective = parse_objective(objective_name), metric = parse_metric(metric_name);
    Input p = read_input(pred, "pred", false, "eval_metric_host", false);
    require_host(p, "eval_metric_host takes NumPy arrays");
    if (p.shape.empty() || p.shape.size() > 2) fail("pred must be a float32 array of shape (n, D) or (n,)");
    const int n = static_cast<int>(p.shape[0]), D = p.shape.size() == 2 ? static_cast<int>(p.shape[1]) : 1;
    Input t = read_objective_targets(targets, "targets", false, "eval_metric_host", objective, n, D, true);
    require_host(t, "eval_metric_host takes NumPy arrays");
    py::array_t<int64_t> counts = metric_counts_array(objective, metric, std::max(D, 1));
    double value = 0.0;
    check(gbrl_hip_eval_metric_host(p.f32(), t.ptr, n, D, objective, metric, &value, counts.mutable_data()));
    return py::make_tuple(py::float_(value), counts);
}

// ---- ranking objectives on query groups (include/gbrl_hip.h, "Ranking objectives")
bool rank_objective_name(const std::string &s) { return s == "pairwise" || s == "lambdarank"; }
int parse_rank_objective(const std::string &s) {
    return parse_enum(s, {{"pairwise", GBRL_HIP_OBJ_PAIRWISE}, {"lambdarank", GBRL_HIP_OBJ_LAMBDARANK}},
                      "Invalid objective! The ranking objectives are: pairwise/lambdarank");
}
int rank_rows_of(const Input &p, const std::string &fn) {
    const bool ok = (p.shape.size() == 1 && p.shape[0] > 0) || (p.shape.size() == 2 && p.shape[1] == 1 && p.shape[0] > 0);
    if (!ok) fail(fn + ": pred must be float32 of shape (n,) or (n, 1): a ranking objective scores a row with one number");
    return static_cast<int>(p.shape[0]);
}

// rank_gradient(pred, labels, group, objective, ndcg_at) -> dict: NumPy in, NumPy out; a device tuple for pred gives DLPack capsules for grad, hess and positions
py::dict rank_gradient_impl(PyGBRL &self, py::object &pred, py::object &labels, py::object &group, const std::string &objective_name, py::object ndcg_at_obj) {
    const std::string fn = "rank_gradient";
    const int objective = parse_rank_objective(objective_name);
    const int ndcg_at = read_ndcg_at(ndcg_at_obj, fn);
    Input p = require_input(pred, "pred", fn);
    const int n = rank_rows_of(p, fn);
    Input l = read_rank_labels(labels, fn, n);
    const std::vector<int32_t> grp = read_group(group, fn);
    const int Q = static_cast<int>(grp.size());
    py::array_t<double> ndcg(std::vector<py::ssize_t>{Q});
    double loss = 0.0;
    int64_t pairs = 0;
    // grad, hess and positions go where pred lives: the model's device, or the host
    const int dev_id = result_device(self, p.on_device);
    Result<float> g(p.on_device, dev_id, static_cast<size_t>(n)), h(p.on_device, dev_id, static_cast<size_t>(n));
    Result<int32_t> pos(p.on_device, dev_id, static_cast<size_t>(n));
    {
        py::gil_scoped_release release;
        check(gbrl_hip_rank_gradient(self.h, p.f32(), p.on_device, l.i32(), l.on_device, grp.data(), Q, n, objective, ndcg_at, g.get(), h.get(), &loss,
                                      ndcg.mutable_data(), pos.get(), &pairs));
    }
    py::dict out;
    out["grad"] = g.release(shape_of(p));
    out["hess"] = h.release(shape_of(p));
    out["positions"] = pos.release({n});
    out["loss"] = py::float_(loss);
    out["ndcg"] = ndcg;
    out["pairs"] = py::int_(pairs);
    return out;
}

// the rule on the host: no device, no model
py::dict rank_gradient_host_impl(py::object &scores, py::object &labels, py::object &group, const std::string &objective_name, py::object ndcg_at_obj) {
    const std::string fn = "rank_gradient_host";
    const int objective = parse_rank_objective(objective_name);
    const int ndcg_at = read_ndcg_at(ndcg_at_obj, fn);
    Input p = read_input(scores, "scores", false, fn, false);
    require_host(p, "rank_gradient_host takes NumPy arrays");
    const int n = rank_rows_of(p, fn);
    Input l = read_rank_labels(labels, fn, n);
    require_host(l, "rank_gradient_host takes NumPy arrays");
    const std::vector<int32_t> grp = read_group(group, fn);
    const int Q = static_cast<int>(grp.size());
    py::array_t<float> g(std::vector<py::ssize_t>(p.shape.begin(), p.shape.end())), h(std::vector<py::ssize_t>(p.shape.begin(), p.shape.end()));
    py::array_t<int32_t> pos(std::vector<py::ssize_t>{n});
    py::array_t<double> ndcg(std::vector<py::ssize_t>{Q});
    double loss = 0.0;
    int64_t pairs = 0;
    const bool with_loss = objective == GBRL_HIP_OBJ_LAMBDARANK;
    check(gbrl_hip_rank_gradient_host(p.f32(), l.i32(), grp.data(), Q, n, objective, ndcg_at, g.mutable_data(),
                                      h.mutable_data(), with_loss ? &loss : nullptr, ndcg.mutable_data(), pos.mutable_data(), &pairs));
    py::dict out;
    out["grad"] = g;
    out["hess"] = h;
    if (with_loss) out["loss"] = py::float_(loss);
    out["ndcg"] = ndcg;
    out["positions"] = pos;
    out["pairs"] = py::int_(pairs);
    return out;
}

py::array_t<double> rank_discounts_impl() {
    int cap = 0;
    gbrl_hip_rank_geometry(&cap, nullptr);
    py::array_t<double> out(std::vector<py::ssize_t>{cap});
    check(gbrl_hip_rank_discounts(out.mutable_data()));
    return out;
}

py::dict rank_geometry_impl() {
    int cap = 0, label = 0;
    gbrl_hip_rank_geometry(&cap, &label);
    py::dict out;
    out["max_query"] = cap;
    out["max_label"] = label;
    return out;
}

py::object objective_exp_host_impl(py::array_t<float, py::array::c_style | py::array::forcecast> t, bool rounded) {
    const std::vector<py::ssize_t> shape(t.shape(), t.shape() + t.ndim());
    float none = 0.0f;
    if (rounded) {
        py::array_t<float> out(shape);
        check(gbrl_hip_objective_exp_host(t.size() ? t.data() : &none, static_cast<int>(t.size()), nullptr, t.size() ? out.mutable_data() : &none));
        return std::move(out);
    }
    py::array_t<double> out(shape);
    double none64 = 0.0;
    check(gbrl_hip_objective_exp_host(t.size() ? t.data() : &none, static_cast<int>(t.size()), t.size() ? out.mutable_data() : &none64, nullptr));
    return std::move(out);
}

// objective_gradient(pred, targets, objective, weights=None) -> (grad, loss): NumPy in, NumPy out; a device tuple gives a DLPack capsule on the model's device
py::tuple objective_gradient_impl(PyGBRL &self, py::object &pred, py::object &targets, const std::string &objective_name, py::object &weights, py::object alpha_obj,
                                  py::object group, py::object ndcg_at) {
    if (rank_objective_name(objective_name)) {   // the ranking objectives: targets are the int32 labels, the rows of a query are named by group
        if (!weights.is_none() || !alpha_obj.is_none()) fail("objective_gradient: weights and alpha do not go with a ranking objective");
        py::dict r = rank_gradient_impl(self, pred, targets, group, objective_name, ndcg_at);
        return py::make_tuple(r["grad"], r["loss"]);
    }
    if (!group.is_none() || !ndcg_at.is_none()) fail("objective_gradient: group and ndcg_at belong to the ranking objectives 'pairwise' and 'lambdarank'");
    const gbrl_hip_metadata md = self.meta();
    const int objective = parse_objective(objective_name), D = md.output_dim;
    const std::vector<float> alpha = read_alpha(alpha_obj, D, "objective_gradient");
    Input p = require_input(pred, "pred", "objective_gradient");
    const int n = p.shape.empty() ? 0 : static_cast<int>(p.shape[0]);
    check_rows_by_outputs(p, "pred", n, D);
    Input t = read_objective_targets(targets, "targets", false, "objective_gradient", objective, n, D, true);
    if (!t.ptr) fail("Cannot call objective_gradient without targets!");
    Input w = read_weights(weights, "weights", "objective_gradient", n, true);
    if (w.ptr && (objective == GBRL_HIP_OBJ_QUANTILE || !alpha.empty())) fail("objective_gradient: row weights with the quantile objective (alpha=) are not supported");
    Result<float> g(p.on_device, result_device(self, p.on_device), std::max<size_t>(static_cast<size_t>(n) * D, 1));   // where pred lives
    double loss = 0.0;
    {
        py::gil_scoped_release release;
        if (objective == GBRL_HIP_OBJ_QUANTILE || !alpha.empty())
            check(gbrl_hip_objective_gradient_quantile(self.h, p.f32(), p.on_device, t.ptr, t.on_device, alpha.empty() ? nullptr : alpha.data(),
                                                       n, objective, g.get(), &loss));
        else
            check(gbrl_hip_objective_gradient_weighted(self.h, p.f32(), p.on_device, t.ptr, t.on_device, w.f32(), w.on_device, n, objective, g.get(), &loss));
    }
    return py::make_tuple(g.release(shape_of(p)), py::float_(loss));
}

// the gradient rule on the host (include/gbrl_hip.h, "Classification objectives"): no device, no model
py::array_t<float> objective_gradient_host_impl(py::object &pred, py::object &targets, const std::string &objective_name, py::object &weights, py::object alpha_obj) {
    const int objective = parse_objective(objective_name);
    Input p = read_input(pred, "pred", false, "objective_gradient_host", false);
    require_host(p, "objective_gradient_host takes NumPy arrays");
    if (p.shape.empty() || p.shape.size() > 2) fail("pred must be a float32 array of shape (n, D) or (n,)");
    const int n = static_cast<int>(p.shape[0]), D = p.shape.size() == 2 ? static_cast<int>(p.shape[1]) : 1;
    Input t = read_objective_targets(targets, "targets", false, "objective_gradient_host", objective, n, D, true);
    require_host(t, "objective_gradient_host takes NumPy arrays");
    Input w = read_weights(weights, "weights", "objective_gradient_host", n, true);
    require_host(w, "objective_gradient_host takes NumPy arrays");
    const std::vector<float> alpha = read_alpha(alpha_obj, D, "objective_gradient_host");
    py::array_t<float> out(std::vector<py::ssize_t>(p.shape.begin(), p.shape.end()));
    float none = 0.0f;
    if (objective == GBRL_HIP_OBJ_QUANTILE || !alpha.empty()) {
        if (w.ptr) fail("objective_gradient_host: row weights with the quantile objective (alpha=) are not supported");
        check(gbrl_hip_objective_gradient_host_quantile(p.f32(), t.ptr, alpha.empty() ? nullptr : alpha.data(), n, D, objective,
                                                        out.size() ? out.mutable_data() : &none));
        return out;
    }
    check(gbrl_hip_objective_gradient_host_weighted(p.f32(), t.ptr, w.f32(), n, D, objective, out.size() ? out.mutable_data() : &none));
    return out;
}

// ---- feature importance (include/gbrl_hip.h, "Feature importance")
// permutation_host(n, seed=0, col=0, repeat=0) -> int32 [n]: the rule on the host, no device
py::array_t<int32_t> permutation_host_impl(int n, uint64_t seed, int col, int repeat) {
    py::array_t<int32_t> out(static_cast<py::ssize_t>(std::max(n, 0)));
    int32_t none = 0;
    check(gbrl_hip_permutation_host(n, seed, col, repeat, n > 0 ? out.mutable_data() : &none));
    return out;
}

py::dict permutation_geometry_impl() {
    int variants = 0, rows = 0;
    gbrl_hip_permutation_geometry(&variants, &rows);
    py::dict out;
    out["launch_variants"] = variants;
    out["tile_rows"] = rows;
    return out;
}

// permutation_importance_prepared(ds, targets, objective='rmse', n_repeats=5, seed=0, cols=None, n_trees=None, alpha=None) -> dict
py::dict permutation_importance_prepared_impl(PyGBRL &self, py::object ds_obj, py::object &targets, const std::string &objective_name, int n_repeats, uint64_t seed,
                                              py::object &cols, py::object n_trees_obj, py::object alpha_obj) {
    const std::string fn = "permutation_importance_prepared";
    const gbrl_hip_metadata md = self.meta();
    const gbrl_hip_dataset *ds = dataset_handle(ds_obj);
    const int objective = parse_objective(objective_name), D = md.output_dim;
    if (n_repeats < 1) fail(fn + ": n_repeats must be >= 1, got " + std::to_string(n_repeats));
    int n_trees = -1;   // None: every tree
    if (!n_trees_obj.is_none()) {
        const long long k = n_trees_obj.cast<long long>();
        if (k < 1 || k > md.n_trees)
            fail(fn + ": n_trees " + std::to_string(k) + " is outside [1, " + std::to_string(md.n_trees) + "], the model's trees (None / -1: all)");
        n_trees = static_cast<int>(k);
    }
    const gbrl_hip_dataset_desc info = dataset_info(ds_obj);
    const int n = info.n_rows, F = info.n_features;
    std::vector<int32_t> cv;
    if (!cols.is_none()) {
        cv = read_cols(cols, fn);
        if (cv.empty()) fail(fn + ": cols must name between 1 and " + std::to_string(F) + " columns, got 0");
    } else {
        cv.resize(static_cast<size_t>(F));
        for (int f = 0; f < F; ++f) cv[f] = f;
    }
    const std::vector<float> alpha = read_alpha(alpha_obj, D, fn);
    const bool ranking = objective == GBRL_HIP_OBJ_PAIRWISE || objective == GBRL_HIP_OBJ_LAMBDARANK;   // (refused behind the C ABI: no shape of theirs is checked here)
    Input t = read_objective_targets(targets, "targets", false, fn, objective, n, D, ds != nullptr && !ranking);
    if (!t.ptr) fail("Cannot call " + fn + " without targets!");
    const py::ssize_t C = static_cast<py::ssize_t>(cv.size()), R = n_repeats;
    py::array_t<double> loss({std::max<py::ssize_t>(C, 1), R});
    double baseline = 0.0;
    {
        py::gil_scoped_release release;
        check(gbrl_hip_permutation_importance_prepared(self.h, ds, t.ptr, t.on_device, objective, alpha.empty() ? nullptr : alpha.data(), n_repeats, seed,
                                                        cols.is_none() ? nullptr : cv.data(), static_cast<int>(cv.size()), n_trees, &baseline, loss.mutable_data()));
    }
    py::array_t<double> importance({C, R}), mean(C), sd(C);
    py::array_t<int32_t> cols_out(C);
    const double *L = loss.data();
    for (py::ssize_t c = 0; c < C; ++c) {
        cols_out.mutable_data()[c] = cv[static_cast<size_t>(c)];
        double s = 0.0;
        for (py::ssize_t r = 0; r < R; ++r) {
            importance.mutable_data()[c * R + r] = L[c * R + r] - baseline;
            s += importance.data()[c * R + r];
        }
        const double mu = s / static_cast<double>(R);
        double q = 0.0;
        for (py::ssize_t r = 0; r < R; ++r) q += (importance.data()[c * R + r] - mu) * (importance.data()[c * R + r] - mu);
        mean.mutable_data()[c] = mu;
        sd.mutable_data()[c] = std::sqrt(q / static_cast<double>(R));   // the population form, as numpy.std
    }
    py::dict out;
    out["baseline"] = py::float_(baseline);
    out["loss"] = loss;
    out["importance"] = importance;
    out["mean"] = mean;
    out["std"] = sd;
    out["cols"] = cols_out;
    return out;
}

// feature_importance(kind='split' | 'cover', leaf_counts=None) -> float64 [input_dim], from the host copy of the model
py::array_t<double> feature_importance_impl(PyGBRL &self, const std::string &kind_name, py::object leaf_counts) {
    const gbrl_hip_metadata md = self.meta();
    const int kind = parse_enum(kind_name, {{"split", GBRL_HIP_IMPORTANCE_SPLIT}, {"cover", GBRL_HIP_IMPORTANCE_COVER}}, "Invalid kind! Options are: split/cover");
    py::array_t<int64_t, py::array::c_style | py::array::forcecast> counts;
    if (kind == GBRL_HIP_IMPORTANCE_COVER) {
        if (leaf_counts.is_none()) fail("feature_importance: kind 'cover' needs leaf_counts, the int64 vector GBRL.leaf_counts returns");
        counts = py::array_t<int64_t, py::array::c_style | py::array::forcecast>::ensure(leaf_counts);
        if (!counts) { PyErr_Clear(); fail("feature_importance: leaf_counts must be a vector of integers"); }
        if (counts.ndim() != 1 || counts.shape(0) != md.n_leaves)
            fail("feature_importance: leaf_counts must hold one count per leaf of the ensemble (" + std::to_string(md.n_leaves) + ")");
    }
    py::array_t<double> out(static_cast<py::ssize_t>(md.input_dim));
    double none = 0.0;
    check(gbrl_hip_feature_importance(self.h, kind, kind == GBRL_HIP_IMPORTANCE_COVER ? counts.data() : nullptr, md.input_dim > 0 ? out.mutable_data() : &none));
    return out;
}

// ---- partial dependence and ICE (include/gbrl_hip.h, "Partial dependence")

// partial_dependence_codes(thresholds, col, n_trees=None) -> int32 [k + 1]: the break rule on the host, no device
py::array_t<int32_t> partial_dependence_codes_impl(PyGBRL &self, py::object &thresholds, int col, py::object n_trees_obj) {
    Input t = read_input(thresholds, "thresholds", false, "partial_dependence_codes", false);
    require_host(t, "partial_dependence_codes takes a NumPy array");
    if (t.shape.size() != 2) fail("thresholds must be the [n_features, n_bins] array PreparedDataset.thresholds() returns");
    std::vector<int32_t> buf(t.shape[1] + 1);
    int count = 0;
    check(gbrl_hip_partial_dependence_codes(self.h, t.f32(), static_cast<int>(t.shape[0]), static_cast<int>(t.shape[1]), col,
                                            read_n_trees(n_trees_obj), buf.data(), &count));
    py::array_t<int32_t> out(static_cast<py::ssize_t>(count));
    std::copy(buf.begin(), buf.begin() + count, out.mutable_data());
    return out;
}

py::dict partial_dependence_geometry_impl(int m, int D) {
    int rows = 0, launch = 0, most = 0;
    uint64_t budget = 0;
    gbrl_hip_partial_dependence_geometry(m, D, &rows, &launch, &most, &budget);
    py::dict out;
    out["partial_rows"] = rows;
    out["launch_variants"] = launch;
    out["max_launch_variants"] = most;
    out["scratch_budget"] = py::int_(budget);
    return out;
}

const std::string kPdFn = "partial_dependence_prepared";

// partial_dependence_prepared in four stages -- the entries, the breaks of a column, the cell list, the shaped result -- and what they hand on
struct PdPlan {
    struct Entry { int c0, c1; };   // a column, or (c1 >= 0) a pair of two distinct columns
    gbrl_hip_model *model = nullptr;
    int F = 0, B = 0, n_trees = -1;
    std::vector<Entry> entries;
    std::vector<float> thr;                                   // the data set's thresholds [F, B]
    std::unordered_map<int, std::vector<int32_t>> codes;      // the breaks of every named column
    std::vector<int32_t> variants{-1, 0, -1, 0};              // pd_core.h's cell list, four ints per variant; variant 0 is the baseline
    std::vector<size_t> first;                                // the first variant of every entry
};

// the entries: an int column, or a pair of two distinct columns
void pd_read_entries(PdPlan &p, py::object &features, long long max_cells) {
    const std::string &fn = kPdFn;
    const int F = p.F;
    if (!py::isinstance<py::sequence>(features) || py::isinstance<py::str>(features)) fail(fn + ": features must be a sequence of columns and (c0, c1) pairs");
    auto column = [&](py::handle h, size_t e) {
        if (!py::isinstance<py::int_>(h) && !(py::hasattr(h, "__index__") && !py::isinstance<py::float_>(h))) fail(fn + ": entry " + std::to_string(e) + " of features is neither a column nor a pair of columns");
        const long long c = py::reinterpret_steal<py::object>(PyNumber_Index(h.ptr())).cast<long long>();
        if (c < 0 || c >= F) fail(fn + ": entry " + std::to_string(e) + " of features names column " + std::to_string(c) + ", outside [0, " + std::to_string(F) + ")");
        return static_cast<int>(c);
    };
    size_t e = 0;
    for (py::handle h : features.cast<py::sequence>()) {
        if (py::isinstance<py::sequence>(h) && !py::isinstance<py::str>(h)) {
            py::sequence pr = py::reinterpret_borrow<py::sequence>(h);
            if (py::len(pr) != 2) fail(fn + ": entry " + std::to_string(e) + " of features has " + std::to_string(py::len(pr)) + " columns: a pair has two");
            const int c0 = column(pr[0], e), c1 = column(pr[1], e);
            if (c0 == c1) fail(fn + ": entry " + std::to_string(e) + " of features names column " + std::to_string(c0) + " twice: a pair needs two distinct columns");
            p.entries.push_back({c0, c1});
        } else {
            p.entries.push_back({column(h, e), -1});
        }
        ++e;
    }
    if (p.entries.empty()) fail(fn + ": features is empty: name at least one column or pair");
    if (max_cells < 1) fail(fn + ": max_cells must be >= 1, got " + std::to_string(max_cells));
}

// the breaks of column c (host only), from the data set's thresholds; worked out when a column is first named
const std::vector<int32_t> &pd_breaks(PdPlan &p, int c) {
    auto it = p.codes.find(c);
    if (it != p.codes.end()) return it->second;
    std::vector<int32_t> buf(static_cast<size_t>(p.B) + 1);
    int count = 0;
    check(gbrl_hip_partial_dependence_codes(p.model, p.thr.data(), p.F, p.B, c, p.n_trees, buf.data(), &count));
    buf.resize(static_cast<size_t>(count));
    return p.codes.emplace(c, std::move(buf)).first->second;
}

// the cells: variant 0 is the baseline, then every entry's cells in order
void pd_cells(PdPlan &p, const gbrl_hip_dataset *ds, long long max_cells) {
    p.thr.resize(static_cast<size_t>(p.F) * p.B);
    check(gbrl_hip_dataset_thresholds(ds, p.thr.data()));
    p.first.resize(p.entries.size());
    for (size_t i = 0; i < p.entries.size(); ++i) {
        const PdPlan::Entry &en = p.entries[i];
        const std::vector<int32_t> &a = pd_breaks(p, en.c0);
        static const std::vector<int32_t> one{0};
        const std::vector<int32_t> &b = en.c1 >= 0 ? pd_breaks(p, en.c1) : one;
        const long long cells = static_cast<long long>(a.size()) * static_cast<long long>(b.size());
        if (cells > max_cells) {
            std::stringstream ss;
            ss << kPdFn << ": entry " << i << " of features (";
            if (en.c1 >= 0) ss << "columns " << en.c0 << " and " << en.c1 << ") has " << a.size() << " x " << b.size() << " = ";
            else ss << "column " << en.c0 << ") has ";
            ss << cells << " cells, max_cells is " << max_cells;
            fail(ss.str());
        }
        p.first[i] = p.variants.size() / 4;
        p.variants.resize(p.variants.size() + 4 * static_cast<size_t>(cells));   // pd_core.h's cell list: one column, or the row-major product of a pair
        check(gbrl_hip_partial_dependence_cells(en.c0, a.data(), static_cast<int>(a.size()), en.c1, en.c1 >= 0 ? b.data() : nullptr, en.c1 >= 0 ? static_cast<int>(b.size()) : 0,
                                                p.variants.data() + 4 * p.first[i]));
    }
}

// the result: sums / m, shaped per entry
py::dict pd_shape_result(const PdPlan &p, const py::array_t<double> &sums, const py::array_t<float> &ice_all, bool ice, py::ssize_t m, int D) {
    const int B = p.B;
    const double *S = sums.data();
    py::array_t<double> baseline(static_cast<py::ssize_t>(D));
    for (int d = 0; d < D; ++d) baseline.mutable_data()[d] = S[d] / static_cast<double>(m);
    py::list l_features, l_codes, l_values, l_pd, l_ice;
    for (size_t i = 0; i < p.entries.size(); ++i) {
        const PdPlan::Entry &en = p.entries[i];
        auto codes_arr = [&](int c) {
            const std::vector<int32_t> &a = p.codes.at(c);
            py::array_t<int32_t> out(static_cast<py::ssize_t>(a.size()));
            std::copy(a.begin(), a.end(), out.mutable_data());
            return out;
        };
        auto values_arr = [&](int c) {   // the threshold segment j >= 1 begins just above: thr[c][codes[j] - 1]
            const std::vector<int32_t> &a = p.codes.at(c);
            py::array_t<float> out(static_cast<py::ssize_t>(a.size() - 1));
            for (size_t j = 1; j < a.size(); ++j) out.mutable_data()[j - 1] = p.thr[static_cast<size_t>(c) * B + static_cast<size_t>(a[j] - 1)];
            return out;
        };
        const py::ssize_t k0 = static_cast<py::ssize_t>(p.codes.at(en.c0).size()), k1 = en.c1 >= 0 ? static_cast<py::ssize_t>(p.codes.at(en.c1).size()) : 1;
        std::vector<py::ssize_t> shape{k0};
        if (en.c1 >= 0) shape.push_back(k1);
        std::vector<py::ssize_t> pd_shape(shape), ice_shape(shape);
        pd_shape.push_back(D);
        ice_shape.push_back(m); ice_shape.push_back(D);
        py::array_t<double> pd(pd_shape);
        const double *src = S + p.first[i] * static_cast<size_t>(D);
        for (py::ssize_t q = 0; q < k0 * k1 * D; ++q) pd.mutable_data()[q] = src[q] / static_cast<double>(m);
        if (en.c1 >= 0) {
            l_features.append(py::make_tuple(en.c0, en.c1));
            l_codes.append(py::make_tuple(codes_arr(en.c0), codes_arr(en.c1)));
            l_values.append(py::make_tuple(values_arr(en.c0), values_arr(en.c1)));
        } else {
            l_features.append(py::int_(en.c0));
            l_codes.append(codes_arr(en.c0));
            l_values.append(values_arr(en.c0));
        }
        l_pd.append(pd);
        if (ice) {
            py::array_t<float> block(ice_shape);
            std::copy_n(ice_all.data() + p.first[i] * static_cast<size_t>(m) * D, static_cast<size_t>(k0 * k1 * m) * D, block.mutable_data());
            l_ice.append(block);
        }
    }
    py::dict out;
    out["features"] = l_features;
    out["rows"] = py::int_(m);
    out["baseline"] = baseline;
    out["codes"] = l_codes;
    out["values"] = l_values;
    out["pd"] = l_pd;
    if (ice) out["ice"] = l_ice;
    return out;
}

// partial_dependence_prepared(ds, features, n_trees=None, rows=None, ice=False, max_cells=4096) -> dict
py::dict partial_dependence_prepared_impl(PyGBRL &self, py::object ds_obj, py::object features, py::object n_trees_obj, py::object &rows, bool ice, long long max_cells) {
    PdPlan p;
    const std::string &fn = kPdFn;
    const gbrl_hip_metadata md = self.meta();
    if (ds_obj.is_none()) fail(fn + ": null data set");
    const PyDataset &pds = ds_obj.cast<const PyDataset &>();
    const gbrl_hip_dataset_desc info = pds.info();
    const int D = md.output_dim;
    p.model = self.h; p.F = info.n_features; p.B = info.n_bins; p.n_trees = read_n_trees(n_trees_obj);
    pd_read_entries(p, features, max_cells);
    pd_cells(p, pds.h, max_cells);
    const size_t V = p.variants.size() / 4;
    if (V > static_cast<size_t>(INT32_MAX)) fail(fn + ": " + std::to_string(V) + " variants do not fit the call's int32 count");   // (the 2^20 bound is the engine's: it counts what it launches)
    Input none;
    const RowsArg r = read_rows_arg(rows, fn, ds_obj, none);
    const py::ssize_t m = std::max(r.m, 0);
    if (ice && static_cast<unsigned long long>(V) * static_cast<unsigned long long>(m) * static_cast<unsigned long long>(D) >= (1ull << 31))
        fail(fn + ": the ICE rows of " + std::to_string(V) + " variants x " + std::to_string(m) + " rows x " + std::to_string(D) +
             " outputs are 2^31 elements or more: pass rows= to evaluate fewer rows, or fewer features per call");
    py::array_t<double> sums({static_cast<py::ssize_t>(V), static_cast<py::ssize_t>(D)});
    py::array_t<float> ice_all;
    if (ice) ice_all = py::array_t<float>({static_cast<py::ssize_t>(V), m, static_cast<py::ssize_t>(D)});
    {
        double *sp = sums.mutable_data();
        float *ip = ice && ice_all.size() > 0 ? ice_all.mutable_data() : nullptr;
        py::gil_scoped_release release;
        check(gbrl_hip_partial_dependence_prepared(self.h, pds.h, p.variants.data(), static_cast<int>(V), r.ptr, r.on_device, r.m, p.n_trees, sp, ip, 0));
    }
    return pd_shape_result(p, sums, ice_all, ice, m, D);
}

float fit_impl(PyGBRL &self, py::object &obs, py::object &cat, py::object &targets, int iterations, bool shuffle,
               const std::string &loss_type) {
    if (loss_type != "MultiRMSE") fail("Invalid loss function! Options are: MultiRMSE");   // stringTolossType, types.cpp:52-56
    const SampleShape s = read_sample_shape(self.meta(), "fit", targets, "targets", "Targets", obs, cat);
    float loss = 0.0f;
    {
        py::gil_scoped_release release;
        check(gbrl_hip_fit(self.h, s.o.f32(), s.o.on_device, s.c.cells(), s.c.on_device, s.first.f32(), s.first.on_device, s.n, s.n_num, s.n_cat, iterations,
                            shuffle ? 1 : 0, &loss));
    }
    return loss;
}

// tree_shap / ensemble_shap (binding.cpp:985-1117): NumPy inputs only, result [n_samples][n_num + n_cat][output_dim].  A HostArray is no Input: it is
// never a device tuple, takes any NumPy array of its type as the reference does (contiguity is refused, not mended) and keeps a signed shape
struct HostArray {
    const void *ptr = nullptr;
    std::vector<py::ssize_t> shape;
    py::object keep;
};
template <typename ArrayT>
HostArray host_array(py::object &obj) {
    HostArray a;
    if (obj.is_none()) return a;
    ArrayT arr = py::cast<ArrayT>(obj);
    if (!arr.attr("flags").attr("c_contiguous").template cast<bool>()) fail("Arrays must be C-contiguous");
    py::buffer_info info = arr.request();
    a.ptr = info.ptr;
    a.shape.assign(info.shape.begin(), info.shape.end());
    a.keep = arr;
    return a;
}

py::array_t<float> shap_impl(PyGBRL &self, bool whole_ensemble, int tree_idx, py::object &obs, py::object &categorical_obs,
                             py::object &norm_values, py::object &base_poly, py::object &offset) {
    const HostArray o = host_array<py::array_t<float>>(obs);
    const HostArray c = host_array<py::array>(categorical_obs);
    const HostArray nv = host_array<py::array_t<float>>(norm_values), bp = host_array<py::array_t<float>>(base_poly),
                    of = host_array<py::array_t<float>>(offset);
    // 1-D inputs are ONE sample (binding.cpp:996-1003, 1014-1021) -- not predict's rule (one_dim_obs: a row or a column), so these lines stay their own
    py::ssize_t n = 0, n_num = 0, n_cat = 0;
    if (o.ptr) { if (o.shape.size() == 1) { n_num = o.shape[0]; n = 1; } else { n_num = o.shape[1]; n = o.shape[0]; } }
    if (c.ptr) {
        if (c.shape.size() == 1) { n_cat = c.shape[0]; if (n == 0) n = 1; } else { n_cat = c.shape[1]; if (n == 0) n = c.shape[0]; }
    }
    const gbrl_hip_metadata md = self.meta();
    // the reference trusts the caller here and reads out of bounds on a mismatch; this build checks
    // (also when the ensemble is empty: predict() may already have latched the feature counts, and the library sizes what it writes from them)
    if ((md.n_trees > 0 || md.n_num_features + md.n_cat_features > 0) && (n_num != md.n_num_features || n_cat != md.n_cat_features))
        fail("Incompatible dimensions");
    const size_t depth = static_cast<size_t>(md.max_depth);
    auto count = [](const HostArray &a) { size_t k = a.ptr ? 1 : 0; for (py::ssize_t d : a.shape) k *= static_cast<size_t>(d); return k; };
    if (count(nv) < (depth + 1) * depth || count(bp) < depth || count(of) < depth * depth)
        fail("norm_values, base_poly and offset must be built for the model's max_depth");
    py::array_t<float> out({n, n_num + n_cat, static_cast<py::ssize_t>(md.output_dim)});
    float *dst = out.mutable_data();
    std::fill(dst, dst + out.size(), 0.0f);
    {
        py::gil_scoped_release release;
        check(whole_ensemble
                   ? gbrl_hip_ensemble_shap(self.h, static_cast<const float *>(o.ptr), static_cast<const char *>(c.ptr), static_cast<int>(n),
                                            static_cast<const float *>(nv.ptr), static_cast<const float *>(bp.ptr), static_cast<const float *>(of.ptr), dst)
                   : gbrl_hip_tree_shap(self.h, tree_idx, static_cast<const float *>(o.ptr), static_cast<const char *>(c.ptr), static_cast<int>(n),
                                        static_cast<const float *>(nv.ptr), static_cast<const float *>(bp.ptr), static_cast<const float *>(of.ptr), dst));
    }
    return out;
}

// shap_prepared / shap_importance_prepared: the three polynomial arrays as ensemble_shap takes them (float32 NumPy), here with exactly max_depth's counts
struct ShapPolyArgs {
    HostArray nv, bp, of;
    const float *norm() const { return static_cast<const float *>(nv.ptr); }
    const float *base() const { return static_cast<const float *>(bp.ptr); }
    const float *offset() const { return static_cast<const float *>(of.ptr); }
};
ShapPolyArgs read_shap_poly(const std::string &fn, int max_depth, py::object &norm_values, py::object &base_poly, py::object &offset) {
    ShapPolyArgs a{host_array<py::array_t<float>>(norm_values), host_array<py::array_t<float>>(base_poly), host_array<py::array_t<float>>(offset)};
    const size_t depth = static_cast<size_t>(max_depth);
    auto count = [](const HostArray &x) { size_t k = 1; for (py::ssize_t d : x.shape) k *= static_cast<size_t>(d); return k; };
    const struct { const HostArray &x; const char *name; size_t want; std::string shape; } all[] = {
        {a.nv, "norm_values", (depth + 1) * depth, "(" + std::to_string(depth + 1) + ", " + std::to_string(depth) + ")"},
        {a.bp, "base_poly", depth, "(" + std::to_string(depth) + ",)"},
        {a.of, "offset", depth * depth, "(" + std::to_string(depth) + ", " + std::to_string(depth) + ")"}};
    for (const auto &e : all) {
        if (!e.x.ptr) fail(fn + ": " + e.name + " is missing (the three polynomial arrays ensemble_shap takes, built for the model's max_depth)");
        if (count(e.x) != e.want)
            fail(fn + ": " + e.name + " has " + std::to_string(count(e.x)) + " elements, the model's max_depth " + std::to_string(depth) + " needs shape " + e.shape);
    }
    return a;
}

// shap_prepared(ds, norm_values, base_poly, offset, rows=None, tree_idx=None) -> float32 [m, F, D]: NumPy for a "cpu" model, a DLPack capsule on the
// model's device for a "cuda" one, as predict delivers
py::object shap_prepared_impl(PyGBRL &self, py::object ds_obj, py::object &norm_values, py::object &base_poly, py::object &offset, py::object &rows,
                              py::object tree_idx_obj) {
    const std::string fn = "shap_prepared";
    const gbrl_hip_metadata md = self.meta();
    if (ds_obj.is_none()) {   // the library's own refusal: what it refuses about the model comes before the missing data set
        check(gbrl_hip_shap_prepared(self.h, nullptr, nullptr, 0, 0, -1, nullptr, nullptr, nullptr, nullptr, 0));
        fail(fn + ": null data set");
    }
    const PyDataset &pds = ds_obj.cast<const PyDataset &>();
    const gbrl_hip_dataset_desc info = pds.info();
    const ShapPolyArgs poly = read_shap_poly(fn, md.max_depth, norm_values, base_poly, offset);
    int tree_idx = -1;
    if (!tree_idx_obj.is_none()) {
        const long long t = tree_idx_obj.cast<long long>();
        if (t < 0 || t >= md.n_trees)   // (-1 means "all" behind the C ABI only: None says it here)
            fail(md.n_trees == 0 ? fn + ": the model has no trees"
                                 : fn + ": tree_idx " + std::to_string(t) + " is outside [0, " + std::to_string(md.n_trees) + "), the model's trees (None: all)");
        tree_idx = static_cast<int>(t);
    }
    Input none;
    const RowsArg r = read_rows_arg(rows, fn, ds_obj, none);
    const int64_t m = std::max(r.m, 0), F = info.n_features, D = md.output_dim;
    // the engine refuses the same (C callers); here too because a "cuda" model allocates its result on the device before the C call
    if (static_cast<unsigned long long>(m) * static_cast<unsigned long long>(F) * static_cast<unsigned long long>(D) >= (1ull << 31))
        fail(fn + ": the matrix of " + std::to_string(m) + " rows x " + std::to_string(F) + " features x " + std::to_string(D) +
             " outputs has 2^31 elements or more: pass rows= to explain fewer rows, or use shap_importance_prepared");
    Result<float> out(self, std::max<size_t>(static_cast<size_t>(m * F * D), 1));
    {
        py::gil_scoped_release release;
        check(gbrl_hip_shap_prepared(self.h, pds.h, r.ptr, r.on_device, r.m, tree_idx, poly.norm(), poly.base(), poly.offset(), out.get(), out.on_device()));
    }
    return out.release({m, F, D});
}

// shap_importance_prepared(ds, norm_values, base_poly, offset, rows=None, chunk_rows=None) -> dict
py::dict shap_importance_prepared_impl(PyGBRL &self, py::object ds_obj, py::object &norm_values, py::object &base_poly, py::object &offset, py::object &rows,
                                       py::object chunk_rows_obj) {
    const std::string fn = "shap_importance_prepared";
    const gbrl_hip_metadata md = self.meta();
    if (ds_obj.is_none()) {   // (as shap_prepared)
        check(gbrl_hip_shap_importance_prepared(self.h, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr));
        fail(fn + ": null data set");
    }
    const PyDataset &pds = ds_obj.cast<const PyDataset &>();
    const gbrl_hip_dataset_desc info = pds.info();
    const ShapPolyArgs poly = read_shap_poly(fn, md.max_depth, norm_values, base_poly, offset);
    int chunk_rows = 0;
    if (!chunk_rows_obj.is_none()) {
        const long long c = chunk_rows_obj.cast<long long>();
        if (c <= 0 || c > INT32_MAX || c % 64 != 0) fail(fn + ": chunk_rows " + std::to_string(c) + " is not a positive multiple of 64 (None: the default)");
        chunk_rows = static_cast<int>(c);
    }
    Input none;
    const RowsArg r = read_rows_arg(rows, fn, ds_obj, none);
    const py::ssize_t F = info.n_features, D = md.output_dim;
    py::array_t<double> sum({F, D}), sum_abs({F, D});
    int used = 0;
    {
        double *sp = sum.mutable_data(), *ap = sum_abs.mutable_data();
        py::gil_scoped_release release;
        check(gbrl_hip_shap_importance_prepared(self.h, pds.h, r.ptr, r.on_device, r.m, poly.norm(), poly.base(), poly.offset(), chunk_rows, sp, ap, &used));
    }
    py::array_t<double> mean({F, D}), mean_abs({F, D});
    for (py::ssize_t i = 0; i < F * D; ++i) {
        mean.mutable_data()[i] = sum.data()[i] / static_cast<double>(r.m);
        mean_abs.mutable_data()[i] = sum_abs.data()[i] / static_cast<double>(r.m);
    }
    py::dict out;
    out["sum"] = sum;
    out["sum_abs"] = sum_abs;
    out["mean"] = mean;
    out["mean_abs"] = mean_abs;
    out["n_rows"] = py::int_(r.m);
    out["chunk_rows"] = py::int_(used);
    return out;
}

// shap_sums_host(phi) -> (sum, sum_abs) float64 [F, D] ([C] for a two-dimensional phi): shap_core.h's reduction rule, no device
py::tuple shap_sums_host_impl(py::array_t<float, py::array::c_style | py::array::forcecast> phi) {
    if (phi.ndim() != 2 && phi.ndim() != 3) fail("shap_sums_host: phi must be float32 [m, F, D] or [m, C]");
    std::vector<py::ssize_t> shape(phi.shape() + 1, phi.shape() + phi.ndim());
    int64_t cols = 1;
    for (py::ssize_t d : shape) cols *= d;
    py::array_t<double> sum(shape), sum_abs(shape);
    check(gbrl_hip_shap_sums_host(phi.data(), phi.shape(0), cols, sum.mutable_data(), sum_abs.mutable_data()));
    return py::make_tuple(sum, sum_abs);
}

py::dict shap_geometry_impl(int F, int D) {
    int tile = 0, chunk = 0;
    uint64_t budget = 0;
    gbrl_hip_shap_geometry(F, D, &tile, &chunk, &budget);
    py::dict out;
    out["tile_rows"] = tile;
    out["default_chunk_rows"] = chunk;
    out["scratch_budget"] = py::int_(budget);
    return out;
}

}  // namespace

PYBIND11_MODULE(gbrl_cpp, m) {
    m.doc() = "MI355X-native drop-in for NVlabs/gbrl's gbrl_cpp (step / predict hot path), backed by libgbrl_hip.so";
    // test helper (gbrl_hip_cat_rank_stats): the device's ranking statistics of a batch's categorical cells -- (feature, first row, count,
    // total) of every distinct (feature, cell) pair
    m.def("_cat_rank_stats", [](py::object cat, py::object grads) {
        Input c = read_input(cat, "cat_obs", false, "_cat_rank_stats", 1);
        Input g = read_input(grads, "grads", false, "_cat_rank_stats", 0);
        if (c.on_device || g.on_device) fail("_cat_rank_stats takes NumPy arrays");
        if (c.shape.empty() || g.shape.empty() || c.shape[0] != g.shape[0] || c.shape[0] == 0) fail("_cat_rank_stats: cat_obs [n, n_cat] and grads [n, output_dim] must have the same n > 0");
        const size_t n = c.shape[0], fc = c.shape.size() > 1 ? c.shape[1] : 1, d = g.shape.size() > 1 ? g.shape[1] : 1;
        if (n * fc >= (size_t(1) << 31) || fc == 0 || d == 0) fail("_cat_rank_stats: shape not supported");
        const int cap = static_cast<int>(std::min<size_t>(n * fc, size_t(1) << 21));
        py::array_t<int32_t> feat(cap), first(cap), count(cap);
        py::array_t<float> total(cap);
        int nd = -1;
        {
            py::gil_scoped_release release;
            check(gbrl_hip_cat_rank_stats(c.cells(), static_cast<int>(n), static_cast<int>(fc), g.f32(),
                                          static_cast<int>(d), cap, feat.mutable_data(), first.mutable_data(), count.mutable_data(), total.mutable_data(), &nd));
        }
        feat.resize({nd}, false); first.resize({nd}, false); count.resize({nd}, false); total.resize({nd}, false);
        return py::make_tuple(feat, first, count, total);
    }, py::arg("categorical_obs"), py::arg("grads"));
    py::class_<PyDataset> pds(m, "PreparedDataset",
                              "A batch of numeric observations binned once (GBRL.prepare_dataset) and stepped on many times (GBRL.step_prepared): thresholds, "
                              "threshold keys and class codes on the device.  Read-only after its creation; several models may share one.");
    pds.def_property_readonly("n_rows", [](const PyDataset &d) { return d.info().n_rows; });
    pds.def_property_readonly("n_features", [](const PyDataset &d) { return d.info().n_features; });
    pds.def_property_readonly("n_bins", [](const PyDataset &d) { return d.info().n_bins; });
    pds.def_property_readonly("generator_type", [](const PyDataset &d) { return std::string(d.info().generator_type == GBRL_HIP_GEN_UNIFORM ? "Uniform" : "Quantile"); });
    pds.def_property_readonly("nbytes", [](const PyDataset &d) { return static_cast<size_t>(d.info().nbytes); });
    pds.def_property_readonly("thresholds_id", [](const PyDataset &d) { return gbrl_hip_dataset_thresholds_id(d.h); },
                              "the id of the data set the thresholds were selected for: its own for a data set made without a reference, the reference's (through "
                              "any chain) for a bound one.  Data sets with the same id share a model's code tables, and fit_prepared(valid=) asks for it.");
    pds.def("_handle", [](const PyDataset &d) { return reinterpret_cast<uintptr_t>(d.h); }, "the gbrl_hip_dataset* of this data set (tests that call the C ABI)");
    pds.def("thresholds", [](const PyDataset &d) {
        const gbrl_hip_dataset_desc i = d.info();
        py::array_t<float> out({static_cast<py::ssize_t>(i.n_features), static_cast<py::ssize_t>(i.n_bins)});
        check(gbrl_hip_dataset_thresholds(d.h, out.mutable_data()));
        return out;
    }, "thresholds() -> float32 [n_features, n_bins]: the split candidates of the batch");
    pds.def("codes", &dataset_codes_impl, py::arg("rows") = py::none(), py::arg("cols") = py::none(),
            "codes(rows=None, cols=None) -> uint16 [ceil(n_features / 16), m, 16]: the class codes, group-major; code of feature f and row r at [f // 16, r, f % 16] =\n"
            "number of thresholds of f below obs[r, f].  rows (int32 vector, NumPy or (ptr, (m,), 'torch.int32', 'cuda'), duplicates allowed): the records of those\n"
            "rows, gathered on the device.  cols (host vector of ints, strictly ascending, in [0, n_features)): the records of that column subset re-packed into\n"
            "ceil(len(cols) / 16) groups -- the code of column cols[s] at [s // 16, j, s % 16], padding slots 0 -- what step_prepared(cols=) grows on.");
    pds.def("sample_cols", [](PyDataset &self, double colsample, uint64_t seed, int draw) { return sample_cols_host_impl(self.info().n_features, colsample, seed, draw); },
            py::arg("colsample"), py::arg("seed") = 0, py::arg("draw") = 0,
            "sample_cols(colsample, seed=0, draw=0) -> int32 NumPy array [k]\n\n"
            "gbrl_cpp.sample_cols_host(n_features, colsample, seed, draw): the columns fit_prepared(colsample=) grows the tree of `draw` on, usable as cols= of\n"
            "step_prepared and codes.");
    pds.def("sample_rows", &dataset_sample_rows_impl, py::arg("subsample"), py::arg("seed") = 0, py::arg("draw") = 0, py::arg("start") = 0,
            py::arg("stop") = py::none(),
            "sample_rows(subsample, seed=0, draw=0, start=0, stop=None) -> DLPack capsule, int32 [m] on the data set's device\n\n"
            "The rows of [start, stop) (stop=None: n_rows) that the row sampler keeps, ascending, as absolute indices: row r is kept iff the 24-bit hash\n"
            "of (seed, draw, r) is below floor(subsample * 2**24) -- gbrl_cpp.sample_rows_host(stop - start, subsample, seed, draw, start) exactly, drawn on\n"
            "the device without atomics (two calls give the same bytes), without replacement.  subsample in [2**-24, 1], seed in [0, 2**64), draw >= 0.\n"
            "torch.from_dlpack(capsule) is usable as rows= of step_prepared and predict_continue_prepared ((t.data_ptr(), (m,), 'torch.int32', 'cuda'));\n"
            "fit_prepared(subsample=) uses draw = the model's tree count before the step.  m may be 0: a tensor of shape (0,).");
    pds.def("sample_goss", &dataset_sample_goss_impl, py::arg("grads"), py::arg("top_rate"), py::arg("other_rate"), py::arg("seed") = 0, py::arg("draw") = 0,
            py::arg("start") = 0, py::arg("stop") = py::none(),
            "sample_goss(grads, top_rate, other_rate, seed=0, draw=0, start=0, stop=None) -> dict\n\n"
            "Gradient-based one-side sampling of the data set rows [start, stop) (stop=None: n_rows) on the device: grads float32 [stop - start, D] (or\n"
            "[stop - start]) are their gradient rows.  Returns 'rows' (int32 [m], absolute, ascending), 'factor' (float32 [m]: 1 for a top row, else\n"
            "fl32((1 - top_rate) / other_rate)), 'grads' (float32 [m, D] shaped like the input: the kept gradient rows with the factor applied), 'n_top'\n"
            "(floor(top_rate * rows)) and 'tau_bits' (the key of the n_top-th largest score; 0x80000000 when n_top == 0) -- gbrl_cpp.goss_rows_host(grads, ...,\n"
            "row0=start) byte for byte.  A NumPy grads gives NumPy arrays; a device tuple gives DLPack capsules on the data set's device (torch.from_dlpack),\n"
            "usable as step_prepared(ds, grads, rows=rows).  The k-th largest score is selected exactly by a radix count on the device; a kept row's position\n"
            "is its rank: two calls return the same bytes.  fit_prepared(goss=) uses draw = the model's tree count before the step.  m may be 0.");
    m.def("sample_rows_host", &sample_rows_host_impl, py::arg("n"), py::arg("subsample"), py::arg("seed") = 0, py::arg("draw") = 0, py::arg("row0") = 0,
          "sample_rows_host(n, subsample, seed=0, draw=0, row0=0) -> int32 NumPy array [m]\n\n"
          "The row sampler's rule on the host (no device is needed): the rows of [row0, row0 + n) that (seed, draw) keeps at `subsample`, ascending.\n"
          "PreparedDataset.sample_rows returns the same list from the device.");
    m.def("goss_rows_host", &goss_rows_host_impl, py::arg("grads"), py::arg("top_rate"), py::arg("other_rate"), py::arg("seed") = 0, py::arg("draw") = 0,
          py::arg("row0") = 0,
          "goss_rows_host(grads, top_rate, other_rate, seed=0, draw=0, row0=0) -> (rows int32 [m], factor float32 [m])\n\n"
          "The one-side sampling rule on the host (no device is needed; include/gbrl_hip.h, 'One-side sampling').  grads float32 [n, D] (or [n]) are the\n"
          "gradient rows of the rows [row0, row0 + n).  score = the float32 sum over d of fl32(g * g), added in order; key = its bits & 0x7FFFFFFF; the k =\n"
          "floor(top_rate * n) rows with the largest keys are top (equal keys by row order: exactly k), factor 1; every other row is kept iff the 24-bit hash\n"
          "of (seed ^ 0x676F737372657374, draw, row) is below floor(other_rate / (1 - top_rate) * 2**24), factor fl32((1 - top_rate) / other_rate).  rows are\n"
          "absolute and ascending.  PreparedDataset.sample_goss returns the same lists, and the gathered gradients, from the device.  Refused: a NaN rate,\n"
          "top_rate outside [0, 1), other_rate outside (0, 1], top_rate + other_rate > 1, other_rate / (1 - top_rate) < 2**-24, row0 < 0, no rows, draw < 0.");
    m.def("objective_gradient_host", &objective_gradient_host_impl, py::arg("pred"), py::arg("targets"), py::arg("objective"), py::arg("weights") = py::none(),
          py::arg("alpha") = py::none(),
          "objective_gradient_host(pred, targets, objective, weights=None, alpha=None) -> float32 NumPy array shaped like pred\n\n"
          "The gradient rule of fit_prepared(objective=) on the host (no device is needed): 'logistic': sigmoid(p) - y, targets float32 like pred;\n"
          "'softmax': softmax(p) - onehot(y), targets int32 [n] labels in [0, D), D >= 2; 'rmse': p - y.  Every float32 step is the one definition the\n"
          "kernels use (an exponential written out in fmaf, correctly rounded division): the device gives the same bits.  weights (float32 [n], every\n"
          "entry finite and in [0, 65536]): fl32(w * g) row by row, one float32 multiply behind the rule; all-ones weights change no bit.\n"
          "'quantile' with alpha (a level in (0, 1), or one per output): x = fl32(p - y), g = 1 - alpha where x > 0, -alpha where x < 0, 0 where x == 0; it takes no\n"
          "weights, and alpha goes with no other objective.");
    m.def("rank_gradient_host", &rank_gradient_host_impl, py::arg("scores"), py::arg("labels"), py::arg("group"), py::arg("objective"), py::arg("ndcg_at") = py::none(),
          "rank_gradient_host(scores, labels, group, objective, ndcg_at=None) -> {'grad', 'hess', 'ndcg', 'positions', 'pairs'} (and 'loss' for 'lambdarank')\n\n"
          "The rule of GBRL.rank_gradient on the host (no device is needed), the one definition the kernels compile too: scores float32 [n], labels int32 [n]\n"
          "in [0, 30], group the query sizes.  positions: pos(i) = #{j of the query: s_j > s_i, or s_j == s_i and j < i}.  For rows i, j of a query with\n"
          "l_i > l_j: delta = fl32(s_i - s_j), rho = objective_gradient_host(-delta, 0, 'logistic'), eta = objective_hessian_host(delta, None, 'logistic');\n"
          "omega = 1 ('pairwise') or (|gain_i - gain_j| * |disc[pos_i] - disc[pos_j]|) * inv with inv = 1 / maxDCG of the query ('lambdarank'; gain(l) =\n"
          "2**l - 1, disc = rank_discounts(), entries at ndcg_at and beyond counted as 0); row i: g -= rho * omega, h += eta * omega; row j: g += rho * omega,\n"
          "h += eta * omega, in float64 from +0.0 with the partners in ascending row order, rounded once to float32.  ndcg: DCG * inv per query (1 where\n"
          "maxDCG is 0).  'loss' is 1 - mean(ndcg) for 'lambdarank'; the pairwise loss is a float64 libm expression computed on the device only.");
    m.def("rank_discounts", &rank_discounts_impl,
          "rank_discounts() -> float64 [1024]: disc[t] = 1 / log2(t + 2), the ONE table the host rule and the kernels of the ranking objectives read");
    m.def("rank_geometry", &rank_geometry_impl, "rank_geometry() -> {'max_query': 1024, 'max_label': 30}: the largest query and relevance label of the ranking objectives");
    m.def("permutation_host", &permutation_host_impl, py::arg("n"), py::arg("seed") = 0, py::arg("col") = 0, py::arg("repeat") = 0,
          "permutation_host(n, seed=0, col=0, repeat=0) -> int32 [n]\n\n"
          "The row permutation of GBRL.permutation_importance_prepared on the host (no device is needed), the one definition the kernels compile too: a\n"
          "bijection pi of [0, n), computed element by element with no state; row i of the variant (col, repeat) reads column col from row pi[i].  A\n"
          "cycle-walking balanced Feistel network: b = max(2, bit_length(n - 1)) rounded up to even, four rounds (L, R) <- (R, L ^ (F_k(R) & (2**(b/2) - 1)))\n"
          "with F_k the row sampler's 24-bit hash keyed by seed ^ 'permutat', col and the round, applied again while the result is >= n.");
    m.def("partial_dependence_geometry", &partial_dependence_geometry_impl, py::arg("m") = 1, py::arg("D") = 1,
          "partial_dependence_geometry(m=1, D=1) -> {'partial_rows': 64, 'launch_variants': ..., 'max_launch_variants': 64, 'scratch_budget': 67108864}: the\n"
          "rows one float64 partial of partial_dependence_prepared sums, the variants one launch takes over m rows of D outputs (its partials, 8 *\n"
          "variants * D * ceil(m / 64) bytes, stay under the budget; never below 1), the most any launch takes, and the budget in bytes.");
    m.def("permutation_geometry", &permutation_geometry_impl,
          "permutation_geometry() -> {'launch_variants': 64, 'tile_rows': 64}: the (column, repeat) variants one launch of permutation_importance_prepared\n"
          "walks, and the rows of its tile (= the rows per loss partial)");
    m.def("shap_sums_host", &shap_sums_host_impl, py::arg("phi"),
          "shap_sums_host(phi) -> (sum, sum_abs), float64 shaped like phi[0]\n\n"
          "The reduction rule of GBRL.shap_importance_prepared on the host (no device is needed): phi float32 [m, F, D] (or [m, C]).  Rows fall into tiles of\n"
          "64; per column a tile's partial is the sequential float64 sum, from 0.0, of its rows in order (sum_abs: of fabs of the float32); the total is the\n"
          "sequential sum of the tile partials in order.  A NaN in a column propagates into that column's two totals and into no other.");
    m.def("shap_geometry", &shap_geometry_impl, py::arg("F") = 1, py::arg("D") = 1,
          "shap_geometry(F=1, D=1) -> {'tile_rows': 64, 'default_chunk_rows': ..., 'scratch_budget': 67108864}: the rows one float64 partial of\n"
          "shap_importance_prepared sums, and its default chunk_rows for F features and D outputs: the largest multiple of 64 whose float32 scratch\n"
          "[chunk_rows, F, D] stays within the budget, and at least 64");
    m.def("leaf_quantile_host", &leaf_quantile_host_impl, py::arg("x"), py::arg("leaves"), py::arg("n_leaves"), py::arg("alpha"),
          "leaf_quantile_host(x, leaves, n_leaves, alpha) -> {'values': float32 [n_leaves, D], 'counts': int64 [n_leaves], 'ranks': int64 [n_leaves, D]}\n\n"
          "The leaf rule of fit_prepared(leaf_update='quantile') and GBRL.quantile_leaves_prepared on the host (no device is needed): x float32 [m, D] are the\n"
          "residuals fl32(p - y), leaves int32 [m] the leaf of every row (an entry outside [0, n_leaves) joins no leaf).  values[leaf, d] is the k-th LARGEST\n"
          "x[:, d] among the rows of the leaf, k = gbrl_cpp.quantile_rank(rows of the leaf, alpha[d]): an element of the data bit for bit, -0.0 taken as +0.0.\n"
          "An empty leaf has count 0, rank 0 and the value 0.  alpha: a level in (0, 1) or one per output.  Refused: a bad level, an x that is not finite.");
    m.def("quantile_rank", [](int64_t rows, float a) {
              int64_t k = 0;
              check(gbrl_hip_quantile_rank(rows, a, &k));
              return k;
          }, py::arg("m"), py::arg("a"),
          "quantile_rank(m, a) -> clamp(ceil(a * m), 1, m) with the product taken exactly (a is the float32 M * 2**-s: 64-bit integers and a shift, never a\n"
          "double product, which can round across an integer): the rank, counted from the smallest residual y - p, that level a selects among m rows.\n"
          "Refused: m outside [1, 2**31 - 1], a level that is not a finite float32 strictly inside (0, 1).");
    m.def("leaf_quantile_geometry", []() {
              int leaves = 0, rows = 0;
              gbrl_hip_leaf_quantile_geometry(&leaves, &rows);
              py::dict d;
              d["max_select_leaves"] = leaves;
              d["rows_per_chunk"] = rows;
              return d;
          }, "leaf_quantile_geometry() -> {'max_select_leaves', 'rows_per_chunk'}: the largest tree quantile_leaves_prepared's select path takes (larger trees are\n"
             "sorted) and the rows one block of its count pass takes at a time, for tests that straddle them.");
    m.def("objective_hessian_host", &objective_hessian_host_impl, py::arg("pred"), py::arg("targets") = py::none(), py::arg("objective") = "logistic",
          py::arg("weights") = py::none(),
          "objective_hessian_host(pred, targets, objective, weights=None) -> float32 NumPy array shaped like pred\n\n"
          "The hessian rule of fit_prepared(leaf_update='newton') on the host (no device is needed): 'logistic': fl32(fl32(1 / (1 + e)) * fl32(e / (1 + e))),\n"
          "e = exp(-|p|) as the gradient computes it; 'softmax': q (1 - q) per class, q as the gradient computes it (the diagonal); 'rmse': 1.  The targets\n"
          "do not enter (None is fine).  weights (float32 [n]): fl32(w * h) row by row.");
    m.def("newton_values_host", &newton_values_host_impl, py::arg("sums"), py::arg("bits"), py::arg("old_values"), py::arg("depths"), py::arg("leaf_l2") = 1.0,
          "newton_values_host(sums, bits, old_values, depths, leaf_l2=1.0) -> float32 [leaves, D]\n\n"
          "The leaf value rule of newton_leaves_prepared on the host: v = (float)((Sg / 2**bits) / (Sh / 2**bits + leaf_l2)) in float64; a leaf with cnt == 0,\n"
          "depth 0 or a denominator that is not positive keeps old_values.  sums int64 [leaves, 2 D + 1] = (Sg, Sh, cnt).");
    m.def("newton_sum_bits", [](int64_t rows, py::object weight_max) {
              if (weight_max.is_none()) return gbrl_hip_newton_sum_bits(rows);
              const int bits = gbrl_hip_newton_sum_bits_weighted(rows, weight_max.cast<float>());
              if (bits < 0) fail(gbrl_hip_last_error());
              return bits;
          }, py::arg("m"), py::arg("weight_max") = py::none(),
          "newton_sum_bits(m, weight_max=None) -> min(40, 62 - bit_length(m) - e): the bits of the quantum newton_leaves_prepared sums m rows in; e is the\n"
          "smallest integer >= 0 with weight_max <= 2**e (None, or a weight_max up to 1: e = 0).  Refused: a weight_max that is NaN, negative or above 65536.");
    m.def("eval_metric_host", &eval_metric_host_impl, py::arg("pred"), py::arg("targets"), py::arg("objective"), py::arg("metric"),
          "eval_metric_host(pred, targets, objective, metric) -> (value, counts)\n\n"
          "The classifier metrics of fit_prepared(eval_metric=) on the host (no device is needed), as include/gbrl_hip.h defines them.  metric 'error':\n"
          "objective 'softmax' (int32 labels [n]) counts the rows whose arg-max (lowest index among equal maxima) is not the label, counts int64 [1];\n"
          "'logistic' (float32 targets like pred) counts the cells with (p > 0) != (y > 0.5) per column, counts int64 [D]; value = wrong / cells.\n"
          "metric 'auc' ('logistic' only): per column the exact AUC with ties counted half, from counts int64 [D, 3] = (2U, P, N): AUC = 2U / (2 P N),\n"
          "value = their mean.  Scores compare through one key (-0.0 == +0.0; a NaN is ordered by its bits: defined, meaningless).  Refused: an unknown\n"
          "name, a metric with 'rmse', 'auc' with 'softmax', a column of one class (named).");
    m.def("objective_exp_host", &objective_exp_host_impl, py::arg("t"), py::arg("rounded") = false,
          "objective_exp_host(t, rounded=False) -> NumPy array shaped like t\n\n"
          "obj_exp of the objectives (include/gbrl_hip.h): exp(t) for t <= 0 in explicit float32 steps, +0 below -104 -- the value p * 2^k itself as\n"
          "float64, or with rounded=True that value rounded once to float32 (obj_exp_f32: what the gradients use).  Diagnostic, host only.");
    m.def("sample_cols_host", &sample_cols_host_impl, py::arg("F"), py::arg("colsample"), py::arg("seed") = 0, py::arg("draw") = 0,
          "sample_cols_host(F, colsample, seed=0, draw=0) -> int32 NumPy array [k]\n\n"
          "The column rule on the host (no device is needed): k = max(1, floor(colsample * F + 0.5)) of the columns 0 .. F - 1, those with the k smallest pairs\n"
          "(u_f, f), u_f the row sampler's 24-bit hash of (seed ^ 0x636F6C73616D706C, draw, f); ascending.  colsample in (0, 1]; 1.0 gives arange(F).");
    py::class_<PyGBRL> g(m, "GBRL");
    g.def(py::init<int, int, int, int, int, int, int, float, std::string, std::string, bool, int, std::string, int, std::string, std::string>(),
          py::arg("input_dim") = 1, py::arg("output_dim") = 1, py::arg("policy_dim") = 1, py::arg("max_depth") = 4,
          py::arg("min_data_in_leaf") = 0, py::arg("n_bins") = 256, py::arg("par_th") = 10, py::arg("cv_beta") = 0.9,
          py::arg("split_score_func") = "cosine", py::arg("generator_type") = "quantile",
          py::arg("use_control_variates") = false, py::arg("batch_size") = 5000, py::arg("grow_policy") = "greedy",
          py::arg("verbose") = 0, py::arg("device") = "cpu", py::arg("learner_name") = "GBRL");
    g.def(py::init<const PyGBRL &>(), py::arg("model"));
    {
        // Addition: the reference's constructor with one more argument, parity_mode, after the reference's own (positional and keyword
        // calls of the reference's signature take the overload above).  The two signature lines above are the reference's, character for
        // character, and tools compare them (tests/test_host.py), so this overload is described in words below them instead of by a third
        // generated line: the docstring so far is kept and the description appended.
        const std::string ref_doc = py::str(g.attr("__init__").attr("__doc__"));
        const std::string doc = ref_doc + "\nAddition (not in the reference): the first form also accepts parity_mode: str = 'default' after learner_name -- "
                                          "'default' | 'reference' | 'exact_argmax', what set_parity_mode(mode) sets.\n";
        py::options opt;
        opt.disable_function_signatures();
        g.def(py::init<int, int, int, int, int, int, int, float, std::string, std::string, bool, int, std::string, int, std::string, std::string, std::string>(),
              doc.c_str(), py::arg("input_dim") = 1, py::arg("output_dim") = 1, py::arg("policy_dim") = 1, py::arg("max_depth") = 4,
              py::arg("min_data_in_leaf") = 0, py::arg("n_bins") = 256, py::arg("par_th") = 10, py::arg("cv_beta") = 0.9,
              py::arg("split_score_func") = "cosine", py::arg("generator_type") = "quantile",
              py::arg("use_control_variates") = false, py::arg("batch_size") = 5000, py::arg("grow_policy") = "greedy",
              py::arg("verbose") = 0, py::arg("device") = "cpu", py::arg("learner_name") = "GBRL", py::arg("parity_mode"));
    }
    g.def_static("load", [](const std::string &filename) {
        gbrl_hip_model *h = gbrl_hip_load(filename.c_str());
        if (!h) fail(gbrl_hip_last_error());
        return new PyGBRL(h);
    }, py::return_value_policy::take_ownership);
    g.def("to_device", [](PyGBRL &self, const std::string &d) { self.device = parse_device(d); }, py::arg("device"));
    g.def("step", &step_impl, py::arg("obs"), py::arg("categorical_obs"), py::arg("grads"));
    {
        // prepare_dataset(obs) keeps its generated signature line (tools and tests compare it); the form with `reference` is a second overload
        // described in words below that line, as the constructor's parity_mode is
        g.def("prepare_dataset", [](PyGBRL &self, py::object &obs) { return prepare_dataset_impl(self, obs); }, py::arg("obs"));
        const std::string sig = py::str(g.attr("prepare_dataset").attr("__doc__"));
        const std::string doc = sig.substr(0, sig.find('\n')) + "\n\n"
            "prepare_dataset(obs, reference=None) -> PreparedDataset\n\n"
            "The numeric preparation of step(obs, None, grads) -- key transpose, split thresholds, class codes, on step's own code paths -- done once and kept on\n"
            "the device.  obs is not needed after the call.  Numeric columns only: categorical split candidates depend on the step's gradients.\n"
            "reference=ds: a data set BOUND to ds's thresholds (LightGBM's Dataset(reference=train)) -- the codes of obs under them, computed in one pass over obs\n"
            "(no transpose, no selection), with its own copies of the thresholds: ds may be destroyed afterwards.  thresholds() returns ds's bytes and\n"
            "thresholds_id is ds's.  It is a full data set: codes(), predict_continue_prepared, step_prepared and fit_prepared work on it, a model grown on ds\n"
            "is accepted on it, and a step on it grows with ds's thresholds.  Refused: a reference whose n_bins, generator_type, width or device is not the model's.";
        py::options opt;
        opt.disable_function_signatures();
        g.def("prepare_dataset", [](PyGBRL &self, py::object &obs, py::object reference) { return prepare_dataset_impl(self, obs, reference); },
              doc.c_str(), py::arg("obs"), py::arg("reference"));
    }
    {
        // step_prepared(ds, grads, rows=None) keeps its generated signature line (tests compare it); the form with cols is a second overload described
        // in words below that line, as prepare_dataset's reference is
        g.def("step_prepared", [](PyGBRL &self, py::object ds, py::object &grads, py::object &rows) { step_prepared_impl(self, ds, grads, rows); }, py::arg("ds"),
              py::arg("grads"), py::arg("rows") = py::none());
        const std::string sig = py::str(g.attr("step_prepared").attr("__doc__"));
        const std::string doc = sig.substr(0, sig.find('\n')) + "\n\n"
            "step_prepared(ds, grads, rows=None, cols=None)\n\n"
            "One boosting step on a prepared data set: with rows=None the model ends up byte for byte as step(obs, None, grads) would leave it, without the\n"
            "transpose, candidates and binning phases.  rows (int32 vector of length m, duplicates allowed, entries in [0, ds.n_rows)): the tree is grown on\n"
            "those rows, grads [m, output_dim] in their order, with the DATA SET'S thresholds (as fit() uses whole-data-set candidates), not the subset's\n"
            "quantiles.  Any model on the same device with the data set's n_bins and generator_type and input_dim == ds.n_features may step on it.\n"
            "cols (host vector of ints, strictly ascending, entries in [0, ds.n_features), at least one): the tree is grown on those columns only -- their\n"
            "histograms are the only ones built.  The model is what a model of input_dim len(cols) with feature weights w[cols] grows on\n"
            "prepare_dataset(obs[:, cols]), with its conditions naming the data set's columns (feature index cols[f']).  The subset's code records (and\n"
            "rows, in the same pass) are gathered on the device: phase 'gather_cols'.  cols naming every column is the call without cols.  Refused before\n"
            "anything changes: unsorted, repeated or out-of-range entries, an empty vector.";
        py::options opt;
        opt.disable_function_signatures();
        g.def("step_prepared", &step_prepared_impl, doc.c_str(), py::arg("ds"), py::arg("grads"), py::arg("rows") = py::none(), py::arg("cols"));
    }
    g.def("condition_bins", &condition_bins_impl, py::arg("thresholds"),
          "condition_bins(thresholds) -> int32 array shaped like get_ensemble_data()['feature_values']\n\n"
          "thresholds: float32 [n_features, n_bins], e.g. PreparedDataset.thresholds().  A used numeric condition x[f] > v gets bin = number of thresholds of f\n"
          "below v, so that x > v <=> code > bin for the data set's codes; unused and categorical slots get -1.  A used value that is not among its feature's\n"
          "thresholds is refused (the message names the tree and the condition).  Host only: no device is needed.");
    g.def("predict_continue_prepared", &predict_continue_prepared_impl, py::arg("ds"), py::arg("base"), py::arg("start_tree_idx") = 0,
          py::arg("stop_tree_idx") = 0, py::arg("rows") = py::none(),
          "predict_continue_prepared(ds, base, start_tree_idx=0, stop_tree_idx=0, rows=None)\n\n"
          "predict_continue(obs[rows], None, base, start_tree_idx, stop_tree_idx) bit for bit, read from the data set's bin codes: obs need not exist any more.\n"
          "base / range / return as predict_continue (a NumPy base gives a new array, a device tuple is updated in place); rows as step_prepared.\n"
          "Every tree of the range must compare against the data set's thresholds (trees grown on it by step_prepared / fit_prepared do).");
    {
        // likewise: fit_prepared(ds, targets, iterations) -> float keeps its generated line; the validation form is the second overload
        g.def("fit_prepared", [](PyGBRL &self, py::object ds, py::object &targets, int iterations) -> float {
            py::object none = py::none();
            return fit_prepared_impl(self, ds, targets, iterations, none, none, 0, 0.0, 1.0, 1.0, 0, "rmse", none, "gradient", 1.0, none, none, none, none, none, none, none).cast<float>();
        }, py::arg("ds"), py::arg("targets"), py::arg("iterations"));
        const std::string sig = py::str(g.attr("fit_prepared").attr("__doc__"));
        const std::string doc = sig.substr(0, sig.find('\n')) + "\n\n"
            "fit_prepared(ds, targets, iterations, valid=None, valid_targets=None, early_stopping_rounds=0, min_delta=0.0, subsample=1.0, colsample=1.0, seed=0,\n"
            "             objective='rmse', eval_metric=None, leaf_update='gradient', leaf_l2=1.0, weights=None, valid_weights=None, goss=None, alpha=None,\n"
            "             group=None, ndcg_at=None, valid_group=None)\n"
            "             -> float | dict\n\n"
            "fit(obs, None, targets, iterations, shuffle=False) on the data set's rows with nothing recomputed: the running prediction is held and advanced by the\n"
            "new trees only, the batch is never binned again.  A fresh model ends up byte for byte as fit() leaves it, with the same loss.  A model with trees\n"
            "keeps its bias and continues from all of them (unlike fit()); they must compare against the data set's thresholds.  No shuffle: permute before\n"
            "prepare_dataset.\n"
            "valid=dsv (a data set with ds's thresholds_id: prepare_dataset(Xv, reference=ds), or ds itself) and valid_targets: returns a dict -- 'loss' (the float\n"
            "above), 'valid_loss' (float64 [iterations + 1]: entry k is staged_loss(Xv, None, valid_targets, stops=[T0 + k])[0] bit for bit, T0 the tree count at\n"
            "entry, evaluated on the device after every iteration), 'iterations' (those run) and 'best_n_trees' (T0 + index of the minimum: the stop_tree_idx to\n"
            "predict with).  Entry k improves iff valid_loss[k] < valid_loss[best] - min_delta; with early_stopping_rounds = R > 0 the loop ends after iteration k\n"
            "when k - best >= R; R = 0 records only.  All trees grown stay in the model (no truncation), which is byte for byte what fit_prepared(ds, targets,\n"
            "iterations run) leaves.  Refused before anything changes: another thresholds_id, valid_targets missing, early_stopping_rounds < 0, min_delta negative\n"
            "or NaN; without valid= the other three must be at their defaults.\n"
            "subsample=p < 1.0 (with or without valid=), seed an int in [0, 2**64): stochastic gradient boosting.  Every tree is grown on a sample of its batch:\n"
            "row r is kept iff the 24-bit hash of (seed, draw, r) is below floor(p * 2**24) (gbrl_cpp.sample_rows_host, PreparedDataset.sample_rows), with draw =\n"
            "the model's tree count before the step, so a fit that is continued continues the sequence and two runs with one seed give the same bytes.  The\n"
            "rows are drawn and their gradient rows gathered on the device in one pass; the tree is what step_prepared(ds, g[rows - start], rows=rows) grows.\n"
            "A draw that keeps no row of the batch takes the whole batch.  A fresh draw per tree, never with replacement.  The returned loss and valid_loss are\n"
            "on all rows, as without sampling.  subsample == 1.0 is the unsampled loop itself, whatever seed is.  Refused before anything changes: a subsample\n"
            "that is NaN or outside [2**-24, 1].\n"
            "colsample=q < 1.0 (with or without subsample and valid=): every tree is grown on k = max(1, floor(q * n_features + 0.5)) of the columns, those\n"
            "gbrl_cpp.sample_cols_host(n_features, q, seed, draw) / ds.sample_cols(q, seed, draw) names at draw = the tree count before the step, with the\n"
            "row sampler's seed; the tree is what step_prepared(..., cols=those) grows, and rows and columns are gathered in one pass.  Trees carry the\n"
            "data set's feature indices; the held prediction, valid_loss and the loss see all columns.  colsample == 1.0 (and a draw of every column, as\n"
            "with one feature) is the call without it: fit_prepared(..., subsample=1.0, seed=0) and fit_prepared(..., subsample=1.0, colsample=1.0, seed=0)\n"
            "run the same code.  Refused before anything changes: a colsample that is NaN or outside (0, 1].\n"
            "objective='logistic' | 'softmax' (with everything above): the loop with that loss in place of MultiRMSE.  logistic: targets float32 [n, D], D\n"
            "independent outputs, g = sigmoid(p) - y.  softmax: targets int32 [n] class labels in [0, D), D >= 2, g = softmax(p) - onehot(y).  The gradient is\n"
            "gbrl_cpp.objective_gradient_host / GBRL.objective_gradient bit for bit, written by the launch that advances the held prediction.  A fresh model's\n"
            "bias is the log odds of the column means (clamped to [1/2n, 1 - 1/2n]) or the log class frequencies (an empty class counts 0.5 rows).  'loss' and\n"
            "'valid_loss' are the mean loss per row (not a square root); predict returns raw scores: apply sigmoid / softmax yourself.  objective='rmse' is\n"
            "the call without the keyword.  Refused before anything changes: an unknown objective, softmax on a model with one output, float targets\n"
            "where labels are wanted and the reverse, a label outside [0, D).\n"
            "eval_metric='error' | 'auc' (with valid= and a classification objective): the dict gains 'valid_metric' (float64 [iterations + 1]: entry k is\n"
            "gbrl_cpp.eval_metric_host of the validation rows' prediction after k iterations, exactly -- the integers are counted on the device behind the\n"
            "validation launch) and 'eval_metric'.  The stopping rule and 'best_n_trees' then follow that curve in place of 'valid_loss' (the error as it is,\n"
            "the AUC negated), 'valid_loss' is recorded as ever, and the model is byte for byte what the call without the keyword leaves after the same\n"
            "number of iterations.  'error': the share of wrong arg-max rows (softmax) or of cells with (p > 0) != (y > 0.5) (logistic); 'auc' (logistic):\n"
            "the mean over the columns of the exact AUC, ties counted half.  Refused before anything changes: eval_metric without valid=, an unknown\n"
            "name, a metric with 'rmse', 'auc' with 'softmax', a column of valid_targets with one class.\n"
            "leaf_update='newton' (with 'logistic' or 'softmax' and everything above), leaf_l2 >= 0: the tree is grown on the gradient as ever, then every leaf\n"
            "stores sum g / (sum h + leaf_l2) over the rows the tree was grown on in place of the mean of g -- h = s (1 - s), or q (1 - q) per class -- the\n"
            "step scikit-learn, XGBoost and LightGBM take.  The sums are exact integers taken on the device over the bin codes (newton_leaves_prepared's\n"
            "kernel, one launch and one read-back per tree), the division is done on the host in float64: the model is byte for byte the loop\n"
            "objective_gradient -> step_prepared -> newton_leaves_prepared -> predict_continue_prepared.  'gradient' is the call without the keyword.\n"
            "Refused before anything changes: an unknown leaf_update, 'newton' with 'rmse', a leaf_l2 that is negative, NaN or infinite, and with\n"
            "'newton' and 'logistic' a target outside [0, 1].\n"
            "weights=w (float32 [n], NumPy or a device tuple; with everything above): one weight per data set row, every entry finite and in [0, 65536], their\n"
            "float64 sum W > 0.  The launch that advances the held prediction stores fl32(w * g): the tree is grown on the weighted gradient.  'loss' is\n"
            "sum w L / W (rmse: sqrt(0.5 sum w L / W)) -- objective_gradient(pred, targets, objective, weights=w)'s loss bit for bit -- and a fresh model's bias is\n"
            "the weighted mean (its log odds; the weighted log class frequencies).  'newton' leaves store sum w g / (sum w h + leaf_l2), the sums' quantum with room\n"
            "for the largest weight ('weight_max' of the dict; gbrl_cpp.newton_sum_bits(m, weight_max)).  valid_weights=wv (float32 [valid rows]) weigh\n"
            "'valid_loss' alone.  All-ones weights give the model, the valid_loss and the loss of the call without the keyword (the rmse loss to one float32 ulp:\n"
            "it is summed by rows).  What weights do NOT do: the split scores see weighted gradients, but their row counts (L2's sum^2 / count,\n"
            "min_data_in_leaf) are unchanged; a gradient leaf stores the mean of w g over its rows, so weights act as gradient multipliers and weights with\n"
            "mean 1 keep the step size; a zero-weight row still counts as a row of its leaf (to drop rows use subsample or step_prepared(rows=)); the metrics\n"
            "stay unweighted.  Refused before anything changes: an entry that is NaN, negative, infinite or above 65536 (the row is named), W == 0, a wrong\n"
            "length or dtype, valid_weights without valid=, valid_weights with eval_metric (not supported).\n"
            "goss=(top_rate, other_rate) (with everything above but subsample < 1): gradient-based one-side sampling, LightGBM's data_sample_strategy='goss'.\n"
            "Every tree is grown on ds.sample_goss(g, top_rate, other_rate, seed, draw, start, stop) of its batch, draw = the tree count before the step: the\n"
            "floor(top_rate * rows) rows with the largest float32 sum of squared gradient entries (ties by row order, exactly that many), and of the rest those\n"
            "whose 24-bit hash is below floor(other_rate / (1 - top_rate) * 2**24) -- a Bernoulli draw like subsample's, not LightGBM's draw of an exact count --\n"
            "with their gradient rows multiplied by fl32((1 - top_rate) / other_rate).  The k-th largest norm is selected on the device and never visits the\n"
            "host.  With weights= the scores are those of fl32(w * g).  'newton' leaves sum over the kept rows with the weights fl32(w * factor) and weight_max =\n"
            "fl32(max w * amp) and are unbiased; a 'gradient' leaf stores the mean of the amplified gradients over the kept rows, about 1 / (top_rate + other_rate)\n"
            "times the batch mean, so such a fit steps that much further per tree (lower the learning rate).  A draw that keeps no row takes the whole batch unamplified.  goss=None is the call without the keyword.  Refused before anything\n"
            "changes: a NaN rate, top_rate outside [0, 1), other_rate outside (0, 1], top_rate + other_rate > 1, other_rate / (1 - top_rate) < 2**-24, goss with\n"
            "subsample < 1, and a largest weight (1 without weights=) whose product with the amplification is above 65536.\n"
            "objective='quantile', alpha=a (a level in (0, 1), broadcast, or a sequence of one level per output; with valid=, subsample, colsample and goss):\n"
            "quantile regression, LightGBM's objective='quantile'.  targets float32 [n, D]; g = 1 - alpha_d where fl32(p - y) > 0, -alpha_d where it is < 0, 0 at\n"
            "0; 'loss' and 'valid_loss' are the mean pinball loss per row; a fresh model's bias is the k-th smallest target of every column, k =\n"
            "gbrl_cpp.quantile_rank(n, alpha_d).  leaf_update='quantile': the tree is grown on that gradient, then every leaf stores, per output, the k-th largest\n"
            "residual fl32(p - y) of the rows the tree was grown on, k from the leaf's row count -- minus the alpha-quantile of y - p (NumPy's\n"
            "method='inverted_cdf'), a minimiser of the leaf's pinball sum, what LightGBM and scikit-learn renew their leaves with -- where a 'gradient' leaf, a\n"
            "mean of values in [-alpha, 1 - alpha], moves the fit by at most the learning rate per tree.  The order statistic is selected exactly on the device\n"
            "(quantile_leaves_prepared's kernels, one enqueue and one read-back per tree): the model is byte for byte the loop objective_gradient ->\n"
            "step_prepared -> quantile_leaves_prepared -> predict_continue_prepared.  Refused before anything changes: 'quantile' without alpha, alpha with\n"
            "another objective, a level outside (0, 1) or NaN (the output is named), a wrong length, leaf_update='quantile' with another objective,\n"
            "leaf_update='newton' with 'quantile' (its hessian is zero), eval_metric with it, a training target that is not finite; not supported:\n"
            "weights= / valid_weights= with it, goss= with leaf_update='quantile' (both would need a weighted quantile).\n"
            "objective='pairwise' | 'lambdarank', group=sizes (with valid=, colsample, early stopping, warm starts and leaf_update='newton'): learning to rank,\n"
            "LightGBM's lambdarank with group=, XGBoost's rank:pairwise and rank:ndcg.  The model has output_dim == 1; targets are int32 relevance labels [n] in\n"
            "[0, 30]; group holds the sizes of the queries' consecutive row runs, each in [1, 1024], summing to n; valid_group likewise for valid=.  The\n"
            "gradient of a row is a sum over the other rows of its query (GBRL.rank_gradient has the rule): 'pairwise' weighs every pair with different labels\n"
            "by 1 -- a query of two rows with labels (1, 0) is the Bradley-Terry preference step -log sigmoid(s_0 - s_1) -- 'lambdarank' by the NDCG change of\n"
            "swapping the two rows; ndcg_at=K counts the discounts of positions K and beyond as 0 (lambdarank only).  Per iteration the held prediction is\n"
            "advanced with no fused gradient, the rank kernels write g (and h), the tree is grown on g, 'newton' leaves store sum g / (sum h + leaf_l2) from\n"
            "those buffers (bits = gbrl_cpp.newton_sum_bits(n, largest query)): the model is byte for byte the loop predict_continue_prepared -> rank_gradient\n"
            "-> step_prepared -> newton_leaves_prepared(group=).  'loss' is rank_gradient's loss of every row, 'valid_loss'[k] that of the validation prediction\n"
            "after k trees: 1 - mean NDCG (lambdarank) or the mean pair loss (pairwise), lower is better.  A fresh model's bias is 0.  Not LightGBM's: no\n"
            "sigmoid parameter, no lambdarank_norm, no position bias, no label_gain.  Refused before anything changes: output_dim != 1, no group, group /\n"
            "valid_group / ndcg_at with another objective, a size outside [1, 1024] (the query is named), sizes that do not sum to the rows, a label outside\n"
            "[0, 30] (the row is named), batch_size < n (a batch must hold whole queries), subsample < 1, goss=, weights= / valid_weights=, alpha=, eval_metric=,\n"
            "leaf_update='quantile', valid= without valid_group, ndcg_at < 0 or with 'pairwise', 'pairwise' on a training set without two different labels in any\n"
            "query.";
        py::options opt;
        opt.disable_function_signatures();
        g.def("fit_prepared", &fit_prepared_impl, doc.c_str(), py::arg("ds"), py::arg("targets"), py::arg("iterations"), py::arg("valid") = py::none(),
              py::arg("valid_targets") = py::none(), py::arg("early_stopping_rounds") = 0, py::arg("min_delta") = 0.0, py::arg("subsample") = 1.0,
              py::arg("colsample") = 1.0, py::arg("seed") = 0, py::arg("objective") = "rmse", py::arg("eval_metric") = py::none(),
              py::arg("leaf_update") = "gradient", py::arg("leaf_l2") = 1.0, py::arg("weights") = py::none(), py::arg("valid_weights") = py::none(),
              py::arg("goss") = py::none(), py::arg("alpha") = py::none(), py::arg("group") = py::none(), py::arg("ndcg_at") = py::none(),
              py::arg("valid_group") = py::none());
    }
    g.def("quantile_leaves_prepared", &quantile_leaves_prepared_impl, py::arg("ds"), py::arg("pred"), py::arg("targets"), py::arg("alpha"), py::arg("rows") = py::none(),
          py::arg("tree") = -1,
          "quantile_leaves_prepared(ds, pred, targets, alpha, rows=None, tree=-1) -> dict\n\n"
          "The leaves of ONE tree (tree=-1: the last) set, per output d, to the k-th largest residual fl32(pred - targets) among the data set rows `rows` (None:\n"
          "every row) the tree routes to the leaf, k = gbrl_cpp.quantile_rank(rows of the leaf, alpha[d]): what fit_prepared(leaf_update='quantile') does after\n"
          "every step.  pred [m, output_dim] is the prediction over the trees before that tree and, like targets (float32 [m, output_dim]), is indexed by\n"
          "position.  alpha: a level in (0, 1) or one per output.  Returns 'values' (float32 [leaves, D], what the model now holds), 'counts' (int64 [leaves])\n"
          "and 'ranks' (int64 [leaves, D]; 0 for an empty leaf).  The value is an element of the data, bit for bit (gbrl_cpp.leaf_quantile_host is the rule):\n"
          "a radix select per (leaf, output) for trees of up to gbrl_cpp.leaf_quantile_geometry()['max_select_leaves'] leaves, a sort by key and leaf beyond --\n"
          "the same bytes.  A leaf without rows or of depth 0 keeps its value.  Refused with the model unchanged: a bad level, a tree outside the model, a\n"
          "prediction, target or residual that is not finite.");
    g.def("newton_leaves_prepared", &newton_leaves_prepared_impl, py::arg("ds"), py::arg("pred"), py::arg("targets"), py::arg("objective"), py::arg("leaf_l2") = 1.0,
          py::arg("rows") = py::none(), py::arg("tree") = -1, py::arg("weights") = py::none(), py::arg("weight_max") = py::none(), py::arg("group") = py::none(),
          py::arg("ndcg_at") = py::none(),
          "newton_leaves_prepared(ds, pred, targets, objective, leaf_l2=1.0, rows=None, tree=-1, weights=None, weight_max=None, group=None, ndcg_at=None) -> dict\n\n"
          "objective 'pairwise' | 'lambdarank' with group= (and ndcg_at=): targets are the int32 relevance labels, g and h are rank_gradient's over every row\n"
          "of the data set (no rows=, no weights=), summed from the buffers its kernels wrote with bits = newton_sum_bits(n, largest query).  Otherwise:\n"
          "The leaves of ONE tree (tree=-1: the last) set to sum g / (sum h + leaf_l2) over the data set rows `rows` (None: every row): what\n"
          "fit_prepared(leaf_update='newton') does after every step.  pred [m, output_dim] is the prediction over the trees before that tree and, like\n"
          "targets (float32 [m, output_dim]; int32 [m] labels for 'softmax'), is indexed by position.  Returns 'sums' (int64 [leaves, 2 D + 1]: Sg, Sh, cnt\n"
          "per leaf, with q(x) = llrint(x * 2**bits)), 'bits' and 'values' (float32 [leaves, D], what the model now holds:\n"
          "gbrl_cpp.newton_values_host(sums, bits, old values, depths, leaf_l2)).  Integer sums: two calls, and both kernel families, give the same bytes.\n"
          "A leaf without rows, of depth 0 or with sum h + leaf_l2 <= 0 keeps its value.  Refused with the model unchanged: 'rmse', a bad leaf_l2, a tree\n"
          "outside the model, a logistic target outside [0, 1], a prediction that is not finite.\n"
          "weights (float32 [m], indexed by position like pred): the sums take q(fl32(w * g)) and q(fl32(w * h)), cnt counts rows, and bits =\n"
          "gbrl_cpp.newton_sum_bits(m, weight_max).  weight_max=None: the largest of the weights given; a loop over sampled rows passes the maximum of the\n"
          "whole data set's weights and gets fit_prepared's bits.  Refused: a bad weight (the row is named), a weight_max below the largest weight given or\n"
          "above 65536, weight_max without weights.");
    g.def("eval_metric", &eval_metric_impl, py::arg("pred"), py::arg("targets"), py::arg("objective"), py::arg("metric"),
          "eval_metric(pred, targets, objective, metric) -> (value, counts)\n\n"
          "gbrl_cpp.eval_metric_host(pred, targets, objective, metric) computed on the model's device: the same integers (counts, int64) and therefore the\n"
          "same value, bit for bit.  pred [n, output_dim] and targets are NumPy arrays or device tuples.  'error' is one launch; 'auc' sorts the score\n"
          "columns with a segmented radix sort, prefix-counts the negatives and sums ranks with integer atomics: two calls give the same bytes.");
    g.def("objective_gradient", &objective_gradient_impl, py::arg("pred"), py::arg("targets"), py::arg("objective"), py::arg("weights") = py::none(),
          py::arg("alpha") = py::none(), py::arg("group") = py::none(), py::arg("ndcg_at") = py::none(),
          "objective_gradient(pred, targets, objective, weights=None, alpha=None, group=None, ndcg_at=None) -> (grad, loss)\n\n"
          "The gradient dL/dp [n, output_dim] and the loss of the raw scores pred under objective 'rmse' | 'logistic' | 'softmax', computed on the model's\n"
          "device by the device functions fit_prepared(objective=) runs: grad is gbrl_cpp.objective_gradient_host(pred, targets, objective) bit for bit.\n"
          "targets: float32 [n, output_dim] (rmse, logistic) or int32 [n] labels (softmax).  NumPy in, NumPy out; a device tuple for pred gives a DLPack\n"
          "capsule.  loss: the mean row loss in float64 (rmse: the MultiRMSE expression), reduced in a fixed order: two calls give the same bits.\n"
          "weights (float32 [n], NumPy or a device tuple, every entry finite and in [0, 65536], sum > 0): grad = fl32(w * g) row by row and loss =\n"
          "sum w L / W with W the float64 sum of the weights in a fixed order (rmse: sqrt(0.5 sum w L / W)); the weight is one more float per row in the\n"
          "same launch.  Refused: a bad entry (the row is named), weights that sum to 0, a wrong length or dtype.\n"
          "'quantile' with alpha (a level in (0, 1) or one per output): the pinball step of gbrl_cpp.objective_gradient_host(..., alpha=) and the mean pinball\n"
          "loss sum_d (u >= 0 ? alpha_d u : (alpha_d - 1) u), u = y - p in float64; no weights with it, alpha with no other objective.\n"
          "'pairwise' | 'lambdarank' with group= (and ndcg_at= for lambdarank): targets are the int32 relevance labels [n] and the call is\n"
          "rank_gradient(pred, targets, group, objective, ndcg_at), of which it returns (grad, loss); group and ndcg_at go with no other objective.");
    g.def("rank_gradient", &rank_gradient_impl, py::arg("pred"), py::arg("labels"), py::arg("group"), py::arg("objective") = "lambdarank", py::arg("ndcg_at") = py::none(),
          "rank_gradient(pred, labels, group, objective='lambdarank', ndcg_at=None) -> {'grad', 'hess', 'loss', 'ndcg', 'positions', 'pairs'}\n\n"
          "The ranking objectives 'pairwise' | 'lambdarank' on query groups, computed on the model's device (output_dim == 1): every figure but the loss is\n"
          "gbrl_cpp.rank_gradient_host(pred, labels, group, objective, ndcg_at) bit for bit.  pred float32 [n] (or [n, 1]) are the scores, labels int32 [n] the\n"
          "relevance grades in [0, 30], group the sizes of the queries' consecutive row runs (each in [1, 1024], summing to n; gbrl_cpp.rank_geometry()).\n"
          "'grad' = dL/dp and 'hess' float32 shaped like pred, 'positions' int32 [n] the 0-based rank of a row inside its query (higher scores first, ties by\n"
          "row order), 'ndcg' float64 [Q] per query, 'pairs' the number P of pairs with different labels inside a query, 'loss' a float: lambdarank\n"
          "1 - mean(ndcg), pairwise the mean of log(1 + exp(-(s_i - s_j))) over the P pairs with l_i > l_j (0 when P == 0), reduced in a fixed order: two calls\n"
          "give the same bits.  A pair with l_i > l_j adds rho = sigmoid(s_j - s_i) times omega to row j's gradient and takes it from row i's, and\n"
          "sigmoid'(s_i - s_j) times omega to both hessians; omega is 1 (pairwise: two rows with labels (1, 0) are the Bradley-Terry step) or\n"
          "|gain_i - gain_j| * |disc[pos_i] - disc[pos_j]| / maxDCG (lambdarank), gain(l) = 2**l - 1, disc = gbrl_cpp.rank_discounts(); ndcg_at=K counts the\n"
          "discount of positions K and beyond as 0 (lambdarank only).  Every row sums its partners in float64, in row order, without atomics.  NumPy in,\n"
          "NumPy out; a device tuple for pred gives DLPack capsules for grad, hess and positions.  Not LightGBM's lambdarank: no sigmoid parameter (it is\n"
          "1), no lambdarank_norm, no position bias, no label_gain table.  Refused: a model with output_dim != 1, a size outside [1, 1024] (the query is\n"
          "named), sizes that do not sum to n, a label outside [0, 30] (the row is named), ndcg_at < 0 or with 'pairwise', a score that is not finite.");
    g.def("predict", [](PyGBRL &self, py::object &obs, py::object &cat, py::object start, py::object stop, bool return_torch) {
        return predict_impl(self, obs, cat, start, stop, return_torch);
    }, py::arg("obs"), py::arg("categorical_obs"), py::arg("start_tree_idx") = 0, py::arg("stop_tree_idx") = 0, py::arg("return_torch") = false);
    // extension (no counterpart in the reference): categorical cells encoded once, predicted many times (include/gbrl_hip.h)
    g.def("encode_categorical", &encode_categorical_impl, py::arg("categorical_obs"));
    g.def("predict_encoded", [](PyGBRL &self, py::object &obs, py::object &ids, uint64_t token, py::object start, py::object stop, bool return_torch) {
        return predict_impl(self, obs, ids, start, stop, return_torch, &token);
    }, py::arg("obs"), py::arg("categorical_ids"), py::arg("dictionary_token"), py::arg("start_tree_idx") = 0, py::arg("stop_tree_idx") = 0,
          py::arg("return_torch") = false);
    // extension: a held prediction carried through the trees grown since (include/gbrl_hip.h)
    g.def("predict_continue", [](PyGBRL &self, py::object &obs, py::object &cat, py::object &base, py::object start, py::object stop) {
        return predict_continue_impl(self, obs, cat, base, start, stop);
    }, py::arg("obs"), py::arg("categorical_obs"), py::arg("base"), py::arg("start_tree_idx") = 0, py::arg("stop_tree_idx") = 0);
    g.def("predict_continue_encoded", [](PyGBRL &self, py::object &obs, py::object &ids, uint64_t token, py::object &base, py::object start, py::object stop) {
        return predict_continue_impl(self, obs, ids, base, start, stop, &token);
    }, py::arg("obs"), py::arg("categorical_ids"), py::arg("dictionary_token"), py::arg("base"), py::arg("start_tree_idx") = 0,
          py::arg("stop_tree_idx") = 0);
    // extension: where a row lands -- the global leaf index per (row, tree), or the rows per leaf reduced on the device
    g.def("predict_leaves", [](PyGBRL &self, py::object &obs, py::object &cat, py::object start, py::object stop) {
        return leaves_impl(self, obs, cat, start, stop, false);
    }, py::arg("obs"), py::arg("categorical_obs"), py::arg("start_tree_idx") = 0, py::arg("stop_tree_idx") = 0);
    g.def("predict_leaves_encoded", [](PyGBRL &self, py::object &obs, py::object &ids, uint64_t token, py::object start, py::object stop) {
        return leaves_impl(self, obs, ids, start, stop, false, &token);
    }, py::arg("obs"), py::arg("categorical_ids"), py::arg("dictionary_token"), py::arg("start_tree_idx") = 0, py::arg("stop_tree_idx") = 0);
    g.def("leaf_counts", [](PyGBRL &self, py::object &obs, py::object &cat, py::object start, py::object stop) {
        return leaves_impl(self, obs, cat, start, stop, true);
    }, py::arg("obs"), py::arg("categorical_obs"), py::arg("start_tree_idx") = 0, py::arg("stop_tree_idx") = 0);
    g.def("leaf_counts_encoded", [](PyGBRL &self, py::object &obs, py::object &ids, uint64_t token, py::object start, py::object stop) {
        return leaves_impl(self, obs, ids, start, stop, true, &token);
    }, py::arg("obs"), py::arg("categorical_ids"), py::arg("dictionary_token"), py::arg("start_tree_idx") = 0, py::arg("stop_tree_idx") = 0);
    g.def_static("leaf_counts_chunk", []() { return gbrl_hip_leaf_counts_chunk(); });   // leaf counters one launch of leaf_counts holds on chip
    // extension: global feature importance -- two counts from the host copy of the model, and the permuted losses of a data set's columns
    g.def("feature_importance", &feature_importance_impl, py::arg("kind") = "split", py::arg("leaf_counts") = py::none(),
          "feature_importance(kind='split', leaf_counts=None) -> float64 [input_dim]\n\n"
          "Counts from the model's structure (no device is needed).  A decision is a level of an oblivious tree (counted once, not once per node) or a\n"
          "distinct internal node of a greedy tree.  'split': the decisions that test the feature.  'cover': sum over leaves of leaf_counts[leaf] * (the\n"
          "conditions on the leaf's path that test the feature) -- the rows reaching every decision on it; leaf_counts is the int64 [n_leaves] vector\n"
          "leaf_counts(obs, categorical_obs) returns.  The feature axis is ensemble_shap's: a condition counts at its raw feature index as\n"
          "get_ensemble_data()['feature_indices'] holds it, numeric and categorical alike (a categorical condition WITHOUT the numeric-feature offset),\n"
          "and feature_mapping is not applied.  Every value is an integer.  Gain importance is not offered: the model file stores no split gain.");
    g.def("permutation_importance_prepared", &permutation_importance_prepared_impl, py::arg("ds"), py::arg("targets"), py::arg("objective") = "rmse",
          py::arg("n_repeats") = 5, py::arg("seed") = 0, py::arg("cols") = py::none(), py::arg("n_trees") = py::none(), py::arg("alpha") = py::none(),
          "permutation_importance_prepared(ds, targets, objective='rmse', n_repeats=5, seed=0, cols=None, n_trees=None, alpha=None) -> dict\n\n"
          "How much the loss of the trees [0, n_trees) on the data set's rows grows when one column is shuffled.  'baseline': the loss on ds as it is, in\n"
          "the units of fit_prepared's valid_loss for the objective; 'loss' float64 [n_cols, n_repeats]: the same loss with column cols[c] read from row\n"
          "gbrl_cpp.permutation_host(n, seed, cols[c], r)[i] -- bit for bit the valid_loss[0] of fit_prepared(ds, y, 0, valid=prepare_dataset(Xp,\n"
          "reference=ds), valid_targets=y) on the shuffled observations Xp, none of which is built here; 'importance' = loss - baseline; 'mean' and 'std'\n"
          "(numpy.std's population form) over the repeats; 'cols'.  cols=None: every column; n_trees=None: all trees (pass best_n_trees of an\n"
          "early-stopped fit).  objective: 'rmse', 'logistic', 'softmax' (int32 labels) or 'quantile' (with alpha).  A column no tree of the range tests\n"
          "reports the baseline's bits.  The model and the data set are not changed.  Refused before the device is touched: n_repeats < 1, bad cols or\n"
          "n_trees, missing or misshapen targets, a model without trees, the ranking objectives, and what predict_continue_prepared refuses.");
    g.def("partial_dependence_codes", &partial_dependence_codes_impl, py::arg("thresholds"), py::arg("col"), py::arg("n_trees") = py::none(),
          "partial_dependence_codes(thresholds, col, n_trees=None) -> int32 [k + 1]\n\n"
          "The codes of column col at which the trees [0, n_trees) can change their answer (no device is needed): [0] + [bin + 1 for the sorted distinct\n"
          "bins, condition_bins' rule for thresholds, of the numeric conditions on col that the walk reads].  Segment j is the code range [codes[j],\n"
          "codes[j + 1] - 1], the last one runs to n_bins; every code of a segment answers every walked condition on col alike.  A column the walk never\n"
          "tests gives [0].  thresholds: PreparedDataset.thresholds().");
    g.def("partial_dependence_prepared", &partial_dependence_prepared_impl, py::arg("ds"), py::arg("features"), py::arg("n_trees") = py::none(),
          py::arg("rows") = py::none(), py::arg("ice") = false, py::arg("max_cells") = 4096,
          "partial_dependence_prepared(ds, features, n_trees=None, rows=None, ice=False, max_cells=4096) -> dict\n\n"
          "Partial dependence (and, with ice=True, the ICE curves) of the trees [0, n_trees), walked from the bias, on the data set's rows (rows=None: every\n"
          "row; an int32 vector or device tuple as step_prepared takes it, duplicates allowed).  features: a sequence whose entries are a column or a pair\n"
          "(c0, c1) of distinct columns.  The curve is exact and needs no grid: a cell holds its column(s) at the first code of a segment of\n"
          "partial_dependence_codes for every row; a pair's cells are the row-major product of its columns' codes.  Returns 'features', 'rows' (m),\n"
          "'baseline' float64 [D] (no column held), and one item per entry in 'codes' (int32 [k + 1]; a tuple of two for a pair), 'values' (float32 [k]:\n"
          "segment j >= 1 begins just above values[j - 1] = thresholds[c][codes[j] - 1]), 'pd' (float64 [k + 1, D] or [k0 + 1, k1 + 1, D]) and, with ice=True,\n"
          "'ice' (float32 [k + 1, m, D] or [k0 + 1, k1 + 1, m, D]).  The curve at an arbitrary code g is pd[np.searchsorted(codes, g, side='right') - 1].\n"
          "An ICE block is bit for bit predict_continue_prepared(dsc, tile(bias), 0, n_trees) on a data set dsc that really holds the cell's codes; pd is\n"
          "the float64 sum of those rows in a fixed order, divided by m: two calls return the same bytes.  The cell of a column no tree of the range tests\n"
          "is the baseline and reports its bits.  The model and the data set are not changed.  Refused before the device is touched: an empty features, a\n"
          "column outside the data set's, a pair that names a column twice, an entry with more than max_cells cells, more than 2^20 launched variants, ICE rows of 2^31\n"
          "elements or more (pass rows=), a bad n_trees, a model without trees, and what predict_continue_prepared refuses.");
    // extension: every ensemble prefix in one walk -- the prediction, or the MultiRMSE loss against targets, after every stops[s] trees
    g.def("predict_staged", &predict_staged_impl, py::arg("obs"), py::arg("categorical_obs"), py::arg("stops") = py::none());
    g.def("staged_loss", &staged_loss_impl, py::arg("obs"), py::arg("categorical_obs"), py::arg("targets"), py::arg("stops") = py::none());
    // extension: the leaf values of a tree range fitted again on new data, the structure kept; returns the loss of the refitted prefix
    g.def("refit_leaves", &refit_leaves_impl, py::arg("obs"), py::arg("categorical_obs"), py::arg("targets"), py::arg("start_tree_idx") = 0,
          py::arg("stop_tree_idx") = 0, py::arg("decay_rate") = 0.0,
          "refit_leaves(obs, categorical_obs, targets, start_tree_idx=0, stop_tree_idx=0, decay_rate=0.0) -> float\n\n"
          "Fit the leaf values of the trees [start_tree_idx, stop_tree_idx) again on this batch; the structure stays.  stop_tree_idx == 0 means n_trees.\n"
          "New value = decay_rate * old + (1 - decay_rate) * the leaf mean of fit()'s MultiRMSE gradient; a leaf without rows keeps its value.\n"
          "Returns staged_loss(obs, categorical_obs, targets, stops=[stop_tree_idx])[0] of the refitted model.  Trees behind stop_tree_idx are not\n"
          "touched and are stale with respect to the new prefix.");
    g.def("fit", &fit_impl, py::arg("obs"), py::arg("categorical_obs"), py::arg("targets"), py::arg("iterations"),
          py::arg("shuffle") = true, py::arg("loss_type") = "MultiRMSE");
    g.def("set_bias", [](PyGBRL &self, py::object &bias) {
        const gbrl_hip_metadata md = self.meta();
        Input b = read_input(bias, "bias", false, "set_bias", false);
        int n, dim;  // binding.cpp:622-657
        if (b.shape.size() == 1) {
            if (md.output_dim > 1) { n = 1; dim = static_cast<int>(b.shape[0]); } else { n = static_cast<int>(b.shape[0]); dim = 1; }
        } else {
            n = static_cast<int>(b.shape[0]); dim = static_cast<int>(b.shape[1]);
            if (n == md.output_dim && dim == 1) { n = 1; dim = static_cast<int>(b.shape[0]); }
        }
        if (dim != md.output_dim) fail_cat("Targets output dim ", dim, " != correct output dim ", md.output_dim);
        if (n > 1) fail("Set bias with multiple samples is not supported!");
        check(gbrl_hip_set_bias(self.h, b.f32(), md.output_dim, b.on_device));
    });
    g.def("set_feature_weights", [](PyGBRL &self, py::object &w) {
        const gbrl_hip_metadata md = self.meta();
        Input x = read_input(w, "feature_weights", false, "set_feature_weights", false);
        size_t tot = 1;
        for (size_t d : x.shape) tot *= d;
        if (static_cast<int>(tot) != md.input_dim) fail_cat("feature_weights input dim ", tot, " != correct input dim ", md.input_dim);
        check(gbrl_hip_set_feature_weights(self.h, x.f32(), md.input_dim, x.on_device));
    });
    g.def("set_feature_mapping", [](PyGBRL &self, const py::array_t<int> &fm, const py::array_t<bool> &mn) {
        if (!(fm.flags() & py::array::c_style) || !(mn.flags() & py::array::c_style)) fail("Arrays must be C-contiguous");
        if (fm.size() != mn.size()) fail("feature_mapping and mapping_numerics must have the same length");
        check(gbrl_hip_set_feature_mapping(self.h, fm.data(), reinterpret_cast<const uint8_t *>(mn.data()), static_cast<int>(fm.size())));
    });
    g.def("get_bias", [](PyGBRL &self) {
        py::array_t<float> a(self.meta().output_dim);
        gbrl_hip_get_bias(self.h, a.mutable_data());
        return a;
    });
    g.def("get_feature_weights", [](PyGBRL &self) {
        py::array_t<float> a(self.meta().input_dim);
        gbrl_hip_get_feature_weights(self.h, a.mutable_data());
        return a;
    });
    g.def("get_feature_mapping", [](PyGBRL &self) {
        const int in = self.meta().input_dim;
        py::array_t<int> fm(in);
        py::array_t<bool> mn(in);
        gbrl_hip_get_feature_mapping(self.h, fm.mutable_data(), reinterpret_cast<uint8_t *>(mn.mutable_data()));
        return py::make_tuple(fm, mn);
    });
    g.def("get_optimizers", [](PyGBRL &self) {
        py::list out;
        for (int i = 0; i < gbrl_hip_num_optimizers(self.h); ++i) {
            gbrl_hip_optimizer o{};
            gbrl_hip_get_optimizer(self.h, i, &o);
            py::dict d;  // keys as binding.cpp:393-410 (including the reference's "eps]" key)
            d["algo"] = o.algo == GBRL_HIP_ALGO_SGD ? "SGD" : "Adam";
            d["init_lr"] = o.init_lr; d["start_idx"] = o.start_idx; d["stop_idx"] = o.stop_idx;
            d["scheduler_func"] = o.scheduler == GBRL_HIP_SCHED_CONST ? "Const" : "Linear";
            d["stop_lr"] = o.stop_lr; d["T"] = o.T; d["beta_1"] = o.beta_1; d["beta_2"] = o.beta_2; d["eps]"] = o.eps;
            out.append(d);
        }
        return out;
    });
    g.def("set_optimizer", [](PyGBRL &self, const std::string &algo, const std::string &sched, float init_lr, int start_idx,
                              int stop_idx, float stop_lr, int T, float beta_1, float beta_2, float eps, float) {
        gbrl_hip_optimizer o{};
        o.algo = parse_enum(algo, {{"SGD", 0}, {"sgd", 0}, {"Adam", 1}, {"adam", 1}}, "Invalid optimizer algorithm! Options are: SGD/Adam");
        o.scheduler = parse_enum(sched, {{"Const", 0}, {"const", 0}, {"Linear", 1}, {"linear", 1}}, "Invalid scheduler! Options are: Const/Linear");
        o.init_lr = init_lr; o.start_idx = start_idx; o.stop_idx = stop_idx; o.stop_lr = stop_lr; o.T = T;
        o.beta_1 = beta_1; o.beta_2 = beta_2; o.eps = eps;
        check(gbrl_hip_set_optimizer(self.h, &o));
    }, py::arg("algo") = "SGD", py::arg("scheduler") = "const", py::arg("init_lr") = 1.0, py::arg("start_idx") = 0,
       py::arg("stop_idx") = 0, py::arg("stop_lr") = 1.0e-8, py::arg("T") = 10000, py::arg("beta_1") = 0.9,
       py::arg("beta_2") = 0.999, py::arg("eps") = 1.0e-8, py::arg("shrinkage") = 0.0);
    g.def("save", [](PyGBRL &self, const std::string &filename) -> int {
        py::gil_scoped_release release;
        const int rc = gbrl_hip_save(self.h, filename.c_str());
        if (rc != GBRL_HIP_OK) { py::gil_scoped_acquire a; fail(gbrl_hip_last_error()); }
        return 0;
    });
    g.def("export", [](PyGBRL &self, const std::string &filename, const std::string &modelname, const std::string &export_format,
                       const std::string &export_type, const std::string &prefix) -> int {
        {
            py::gil_scoped_release release;
            check(gbrl_hip_export(self.h, filename.c_str(), modelname.c_str(), export_format.c_str(), export_type.c_str(), prefix.c_str()));
        }
        return 0;
    }, py::arg("filename"), py::arg("modelname") = "", py::arg("export_format") = "float", py::arg("export_type") = "full", py::arg("prefix") = "");
    g.def("get_scheduler_lrs", [](PyGBRL &self) {
        const int n = gbrl_hip_num_optimizers(self.h);
        if (n == 0) fail("No optimizers found");
        py::array_t<float> a(n);
        gbrl_hip_get_scheduler_lrs(self.h, a.mutable_data());
        return a;
    });
    g.def("get_num_trees", [](PyGBRL &self) { return self.meta().n_trees; });
    g.def("get_iteration", [](PyGBRL &self) { return self.meta().iteration; });
    g.def("get_metadata", [](PyGBRL &self) {
        const gbrl_hip_metadata md = self.meta();
        py::dict d;  // keys as binding.cpp:309-328
        d["input_dim"] = md.input_dim; d["output_dim"] = md.output_dim; d["policy_dim"] = md.policy_dim;
        d["split_score_func"] = md.split_score_func == GBRL_HIP_SCORE_L2 ? "L2" : "Cosine";
        d["generator_type"] = md.generator_type == GBRL_HIP_GEN_UNIFORM ? "Uniform" : "Quantile";
        d["use_control_variates"] = md.use_cv != 0; d["verbose"] = md.verbose; d["max_depth"] = md.max_depth;
        d["min_data_in_leaf"] = md.min_data_in_leaf; d["n_bins"] = md.n_bins; d["par_th"] = md.par_th;
        d["batch_size"] = md.batch_size;
        d["grow_policy"] = md.grow_policy == GBRL_HIP_GROW_GREEDY ? "Greedy" : "Oblivious";
        d["iteration"] = md.iteration;
        return d;
    });
    g.def("get_ensemble_data", [](PyGBRL &self) {
        const gbrl_hip_metadata md = self.meta();
        const py::ssize_t T = md.n_trees, L = md.n_leaves, S = md.grow_policy == GBRL_HIP_GROW_OBLIVIOUS ? T : L;
        const py::ssize_t MD = md.max_depth, D = md.output_dim, in = md.input_dim;
        py::array_t<int> tree_indices(T), depths(S), fidx({S, MD}), rn(in), rc(in), fm(in);
        py::array_t<float> values({L, D}), fval({S, MD}), ew({L, MD}), bias(D), fw(in);
        py::array_t<bool> isnum({S, MD}), ineq({L, MD}), mn(in);
        py::array cats(py::dtype("S128"), std::vector<py::ssize_t>{S, MD});
        gbrl_hip_get_ensemble(self.h, tree_indices.mutable_data(), depths.mutable_data(), values.mutable_data(), fidx.mutable_data(), fval.mutable_data(),
                              ew.mutable_data(), reinterpret_cast<uint8_t *>(isnum.mutable_data()), reinterpret_cast<uint8_t *>(ineq.mutable_data()),
                              static_cast<char *>(cats.mutable_data()), rn.mutable_data(), rc.mutable_data());
        gbrl_hip_get_bias(self.h, bias.mutable_data());
        gbrl_hip_get_feature_weights(self.h, fw.mutable_data());
        gbrl_hip_get_feature_mapping(self.h, fm.mutable_data(), reinterpret_cast<uint8_t *>(mn.mutable_data()));
        py::dict d;  // keys as binding.cpp:330-390
        d["bias"] = bias; d["feature_mapping"] = fm; d["reverse_num_feature_mapping"] = rn; d["reverse_cat_feature_mapping"] = rc;
        d["feature_weights"] = fw; d["tree_indices"] = tree_indices; d["depths"] = depths; d["values"] = values;
        d["feature_indices"] = fidx; d["feature_values"] = fval; d["edge_weights"] = ew; d["is_numerics"] = isnum;
        d["inequality_directions"] = ineq; d["mapping_numerics"] = mn; d["categorical_values"] = cats;
        d["alloc_data_size"] = gbrl_hip_alloc_data_size(self.h);
        return d;
    });
    g.def("get_device", [](PyGBRL &self) { return std::string(self.device ? "cuda" : "cpu"); });
    g.def("get_learner_name", [](PyGBRL &self) { return std::string(gbrl_hip_learner_name(self.h)); });
    g.def("print_tree", [](PyGBRL &self, int tree_idx) {
        { py::gil_scoped_release release; check(gbrl_hip_print_tree(self.h, tree_idx)); }
    }, py::arg("tree_idx") = -1);
    g.def("tree_shap", [](PyGBRL &self, int tree_idx, py::object &obs, py::object &categorical_obs, py::object &norm_values,
                          py::object &base_poly, py::object &offset) {
        return shap_impl(self, false, tree_idx, obs, categorical_obs, norm_values, base_poly, offset);
    }, py::arg("tree_idx") = 0, py::arg("obs"), py::arg("categorical_obs"), py::arg("norm_values"), py::arg("base_poly"), py::arg("offset"));
    g.def("ensemble_shap", [](PyGBRL &self, py::object &obs, py::object &categorical_obs, py::object &norm_values, py::object &base_poly,
                              py::object &offset) {
        return shap_impl(self, true, 0, obs, categorical_obs, norm_values, base_poly, offset);
    }, py::arg("obs"), py::arg("categorical_obs"), py::arg("norm_values"), py::arg("base_poly"), py::arg("offset"));
    g.def("shap_prepared", &shap_prepared_impl, py::arg("ds"), py::arg("norm_values"), py::arg("base_poly"), py::arg("offset"), py::arg("rows") = py::none(),
          py::arg("tree_idx") = py::none(),
          "shap_prepared(ds, norm_values, base_poly, offset, rows=None, tree_idx=None) -> float32 [m, F, D]\n\n"
          "The SHAP values of the rows of a prepared data set (rows: step_prepared's int32 vector, host or device, duplicates allowed; None: every row),\n"
          "computed from its bin codes on the device: NumPy for a 'cpu' model, a DLPack capsule on the model's device for a 'cuda' one.  Bit for bit\n"
          "ensemble_shap(X[rows], None, norm_values, base_poly, offset) -- with tree_idx=t, tree_shap(t, ...) -- for the X the codes were made from: a\n"
          "condition x > v is decided as code > bin, everything else is the same arithmetic.  The three polynomial arrays are ensemble_shap's.  Refused\n"
          "before the device is touched: what predict_continue_prepared refuses, a model with categorical columns or without trees, tree_idx outside the\n"
          "model, a missing or misshapen polynomial array, a (max_depth, output_dim) without a launch plan, and m * F * D >= 2^31 (pass rows=, or use\n"
          "shap_importance_prepared).");
    g.def("shap_importance_prepared", &shap_importance_prepared_impl, py::arg("ds"), py::arg("norm_values"), py::arg("base_poly"), py::arg("offset"),
          py::arg("rows") = py::none(), py::arg("chunk_rows") = py::none(),
          "shap_importance_prepared(ds, norm_values, base_poly, offset, rows=None, chunk_rows=None) -> dict\n\n"
          "'sum', 'sum_abs', 'mean', 'mean_abs': float64 [F, D], the sums over the m rows of the SHAP values of shap_prepared and of their absolute values,\n"
          "and those sums / m ('mean_abs' is the mean |SHAP| importance); 'n_rows' = m; 'chunk_rows' = the value used.  The [m, F, D] matrix is never held\n"
          "whole: chunk_rows rows at a time (a positive multiple of 64; None: the largest whose float32 scratch stays within 64 MiB) are evaluated and\n"
          "reduced on the device.  The sums follow gbrl_cpp.shap_sums_host's rule on that matrix byte for byte, whatever chunk_rows is.  Refusals as\n"
          "shap_prepared's, without the 2^31 limit.");
    g.def("plot_tree", [](PyGBRL &self, int tree_idx, const std::string &filename) {
        check(gbrl_hip_plot_tree(self.h, tree_idx, filename.c_str()));
    }, py::arg("tree_idx") = -1, py::arg("filename"));
    g.def("print_ensemble_metadata", [](PyGBRL &self) {
        { py::gil_scoped_release release; check(gbrl_hip_print_ensemble_metadata(self.h, self.device ? "cuda" : "cpu")); }
    });
    // GBRL::cuda_available (gbrl.cpp:542-548): here "is a HIP device usable"
    g.def_static("cuda_available", []() { return gbrl_hip_device_count() > 0; });
    // ---- additions (not in the reference) ----
    g.def("set_profiling", [](PyGBRL &self, int level) { check(gbrl_hip_set_profiling(self.h, level)); });   // True == 1
    g.def("last_phase_times", [](PyGBRL &self) {
        const char *names[64];
        float ms[64];
        const int n = gbrl_hip_last_phase_times(self.h, names, ms, 64);
        py::dict d;
        for (int i = 0; i < n && i < 64; ++i) d[names[i]] = ms[i];
        return d;
    });
    // Where the near-tie replay decides (gbrl_hip_set_parity_mode): "default" | "reference" | "exact_argmax"; max_node_rows limits the
    // replayed nodes of "reference" in batches above 65 536 rows (0: every node).  Carried by GBRL(model), not by save / load.
    g.def("set_parity_mode", [](PyGBRL &self, const std::string &mode, int max_node_rows) {
        check(gbrl_hip_set_parity_mode(self.h, parse_parity_mode(mode), max_node_rows));
    }, py::arg("mode"), py::arg("max_node_rows") = 0);
    g.def("get_parity_mode", [](PyGBRL &self) {
        int mode = 0, max_node_rows = 0;
        check(gbrl_hip_get_parity_mode(self.h, &mode, &max_node_rows));
        return py::make_tuple(std::string(parity_mode_name(mode)), max_node_rows);
    });
    g.def("_handle", [](PyGBRL &self) { return reinterpret_cast<uintptr_t>(self.h); },
          "address of the underlying gbrl_hip_model (for ctypes callers, e.g. gbrl_hip_set_collective)");
}
