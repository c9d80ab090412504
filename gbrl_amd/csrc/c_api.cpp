// c_api.cpp -- the extern "C" surface declared in include/gbrl_hip.h.  Exceptions never cross the boundary: they are
// turned into status codes + a thread-local message (the reference throws std::runtime_error at the same places).
#include <memory>
#include <mutex>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include <utility>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <new>
#include <string>

#include "../../include/gbrl_hip.h"
#include "engine.h"
#include "objective_core.h"
#include "metric_core.h"
#include "newton_core.h"
#include "quantile_core.h"
#include "rank_core.h"
#include "pd_core.h"
#include "shap_core.h"
#include "hooks.h"
#include "explain.h"
#include "rccl_dyn.h"

struct gbrl_hip_model {
    gbrl::Engine engine;
    std::vector<const char *> phase_names;
    explicit gbrl_hip_model(const gbrl_hip_config &c) : engine(c) {}
    gbrl_hip_model(gbrl::Model &&m, int dev) : engine(std::move(m), dev) {}
    explicit gbrl_hip_model(const gbrl_hip_model &o) : engine(o.engine) {}
};

struct gbrl_hip_dataset {
    std::unique_ptr<gbrl::PreparedDataset> d;
};

namespace {
thread_local std::string g_err;

template <typename Fn>
int guarded(Fn &&fn) {
    gbrl::hooks::begin_call();   // environment hooks are read at most once per API call (hooks.h)
    try {
        fn();
        return GBRL_HIP_OK;
    } catch (const gbrl::NoDeviceError &e) { g_err = e.what(); return GBRL_HIP_E_NO_DEVICE;
    } catch (const gbrl::HipError &e) { g_err = e.what(); return GBRL_HIP_E_HIP;
    } catch (const gbrl::Unsupported &e) { g_err = e.what(); return GBRL_HIP_E_UNSUPPORTED;
    } catch (const gbrl::InvalidArgument &e) { g_err = e.what(); return GBRL_HIP_E_INVALID;
    } catch (const std::bad_alloc &) { g_err = "out of host memory"; return GBRL_HIP_E_INVALID;
    } catch (const std::exception &e) { g_err = e.what(); return GBRL_HIP_E_INVALID; }
}

thread_local int g_ds_status = GBRL_HIP_OK;   // gbrl_hip_dataset_create returns a handle: its status is kept per thread

struct DatasetRegistry {
    std::mutex mu;
    std::unordered_set<const gbrl_hip_dataset *> live;
};
DatasetRegistry &ds_registry() { static DatasetRegistry *r = new DatasetRegistry(); return *r; }
const gbrl::PreparedDataset &live_dataset(const gbrl_hip_dataset *ds) {
    if (ds) {
        std::lock_guard<std::mutex> lk(ds_registry().mu);
        if (ds_registry().live.count(ds)) return *ds->d;
    }
    throw gbrl::InvalidArgument(ds ? "the data set has been destroyed (or is not a data set of this library)" : "null data set");
}

int copy_in(void *dst, const void *src, size_t bytes, int on_device) {
    if (!on_device) { std::memcpy(dst, src, bytes); return 0; }
    return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
}  // namespace

// Output buffers of predict() on the device are recycled: hipMalloc + hipFree (which synchronises the device) cost about
// a millisecond per call, more than the prediction kernel itself for small ensembles.  A freed buffer is kept (up to a few
// buffers / 1 GiB) and handed out again for a request of the same size class after a device synchronisation, so that no
// consumer kernel of its previous life can still be reading it.
namespace {
struct DevPool {
    struct Buf { void *ptr; size_t cap; int device; };
    std::mutex mu;
    std::unordered_map<void *, Buf> live;               // every buffer handed out
    std::vector<Buf> idle;                              // freed buffers kept for reuse ON THEIR OWN DEVICE
    size_t idle_bytes = 0;
    static constexpr size_t kMaxIdleBytes = size_t(1) << 30;
    static constexpr size_t kMaxIdle = 8;
    ~DevPool() { /* process exit: the runtime reclaims device memory; calling hipFree here can race with its teardown */ }
};
DevPool &pool() { static DevPool *p = new DevPool(); return *p; }

// RAII: make `device` current for the calling thread, restore the previous one afterwards
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (device >= 0 && device != prev) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace


extern "C" {

int gbrl_hip_abi_version(void) { return GBRL_HIP_ABI_VERSION; }

int gbrl_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *gbrl_hip_last_error(void) { return g_err.c_str(); }

void *gbrl_hip_device_alloc_on(int device, size_t bytes) {
    if (bytes == 0) bytes = 1;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) { g_err = "no HIP device"; return nullptr; }
    DeviceScope scope(device);
    DevPool &P = pool();
    {
        std::lock_guard<std::mutex> lk(P.mu);
        for (size_t i = 0; i < P.idle.size(); ++i) {
            if (P.idle[i].device == device && P.idle[i].cap >= bytes && P.idle[i].cap <= bytes + bytes / 4 + 4096) {
                const DevPool::Buf b = P.idle[i];
                P.idle_bytes -= b.cap;
                P.idle.erase(P.idle.begin() + static_cast<long>(i));
                P.live[b.ptr] = b;
                (void)hipDeviceSynchronize();   // of `device` (current in this scope): no consumer of the buffer's previous life is still reading it
                return b.ptr;
            }
        }
    }
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        // memory pressure: drop this device's idle buffers and retry once
        std::vector<DevPool::Buf> drop;
        {
            std::lock_guard<std::mutex> lk(P.mu);
            for (size_t i = 0; i < P.idle.size();) {
                if (P.idle[i].device == device) { drop.push_back(P.idle[i]); P.idle_bytes -= P.idle[i].cap; P.idle.erase(P.idle.begin() + static_cast<long>(i)); }
                else ++i;
            }
        }
        for (auto &d : drop) (void)hipFree(d.ptr);
        if (hipMalloc(&p, bytes) != hipSuccess) { g_err = "hipMalloc failed"; return nullptr; }
    }
    std::lock_guard<std::mutex> lk(P.mu);
    P.live[p] = DevPool::Buf{p, bytes, device};
    return p;
}
void *gbrl_hip_device_alloc(size_t bytes) { return gbrl_hip_device_alloc_on(-1, bytes); }
void gbrl_hip_device_free(void *ptr) {
    if (!ptr) return;
    DevPool &P = pool();
    int device = -1;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        auto it = P.live.find(ptr);
        if (it != P.live.end()) {
            const DevPool::Buf b = it->second;
            device = b.device;
            P.live.erase(it);
            if (P.idle.size() < DevPool::kMaxIdle && P.idle_bytes + b.cap <= DevPool::kMaxIdleBytes) {
                P.idle.push_back(b);
                P.idle_bytes += b.cap;
                return;
            }
        }
    }
    DeviceScope scope(device);
    (void)hipFree(ptr);
}

int gbrl_hip_device_ordinal(gbrl_hip_model *m) {
    int dev = -1;
    (void)guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        dev = m->engine.device_ordinal();
    });
    return dev;
}

int gbrl_hip_set_stream(gbrl_hip_model *m, void *hip_stream) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.set_stream(static_cast<hipStream_t>(hip_stream));
    });
}

gbrl_hip_model *gbrl_hip_create(const gbrl_hip_config *cfg) {
    gbrl_hip_model *m = nullptr;
    guarded([&] {
        if (!cfg) throw gbrl::InvalidArgument("null config");
        if (cfg->input_dim <= 0 || cfg->output_dim <= 0 || cfg->max_depth < 0 || cfg->max_depth > 30 || cfg->n_bins <= 0)
            throw gbrl::InvalidArgument("invalid model dimensions");
        if (cfg->use_control_variates)
            throw gbrl::Unsupported("control variates are CPU-only in the reference (gbrl.cpp:204-207) and not part of this build");
        if (cfg->split_score_func != GBRL_HIP_SCORE_L2 && cfg->split_score_func != GBRL_HIP_SCORE_COSINE)
            throw gbrl::InvalidArgument("Invalid score function! Options are: Cosine/L2");
        if (cfg->generator_type != GBRL_HIP_GEN_UNIFORM && cfg->generator_type != GBRL_HIP_GEN_QUANTILE)
            throw gbrl::InvalidArgument("Invalid generator function! Options are: Uniform/Quantile");
        if (cfg->grow_policy != GBRL_HIP_GROW_GREEDY && cfg->grow_policy != GBRL_HIP_GROW_OBLIVIOUS)
            throw gbrl::InvalidArgument("Invalid generator function! Options are: Greedy/Oblivious");
        m = new gbrl_hip_model(*cfg);
    });
    return m;
}

gbrl_hip_model *gbrl_hip_clone(const gbrl_hip_model *other) {
    gbrl_hip_model *m = nullptr;
    guarded([&] {
        if (!other) throw gbrl::InvalidArgument("null model");
        m = new gbrl_hip_model(*other);
    });
    return m;
}

gbrl_hip_model *gbrl_hip_load(const char *filename) {
    gbrl_hip_model *m = nullptr;
    int rc = guarded([&] {
        if (!filename) throw gbrl::InvalidArgument("null filename");
        m = new gbrl_hip_model(gbrl::Model::load(filename), -1);
    });
    if (rc != 0 && g_err.find("file") != std::string::npos) { /* message already set */ }
    return m;
}

int gbrl_hip_save(gbrl_hip_model *m, const char *filename) {
    int rc = guarded([&] {
        if (!m || !filename) throw gbrl::InvalidArgument("null argument");
        m->engine.model.save(filename);
    });
    return rc == GBRL_HIP_OK ? rc : GBRL_HIP_E_IO;
}

void gbrl_hip_destroy(gbrl_hip_model *m) { delete m; }

int gbrl_hip_set_bias(gbrl_hip_model *m, const float *bias, int n, int on_device) {
    return guarded([&] {
        if (!m || !bias) throw gbrl::InvalidArgument("null argument");
        if (n != m->engine.model.meta.output_dim) throw gbrl::InvalidArgument("Incompatible dimensions");
        if (copy_in(m->engine.model.bias.data(), bias, sizeof(float) * n, on_device)) throw gbrl::HipError("hipMemcpy failed");
        ++m->engine.model.version;
    });
}

int gbrl_hip_set_feature_weights(gbrl_hip_model *m, const float *w, int n, int on_device) {
    return guarded([&] {
        if (!m || !w) throw gbrl::InvalidArgument("null argument");
        if (n != m->engine.model.meta.input_dim) throw gbrl::InvalidArgument("Incompatible dimensions");
        if (copy_in(m->engine.model.feature_weights.data(), w, sizeof(float) * n, on_device)) throw gbrl::HipError("hipMemcpy failed");
        ++m->engine.model.version;
    });
}

int gbrl_hip_set_feature_mapping(gbrl_hip_model *m, const int32_t *feature_mapping, const uint8_t *mapping_numerics, int n) {
    return guarded([&] {
        if (!m || !feature_mapping || !mapping_numerics) throw gbrl::InvalidArgument("null argument");
        if (n != m->engine.model.meta.input_dim) throw gbrl::InvalidArgument("Incompatible dimensions");
        m->engine.model.set_feature_mapping(feature_mapping, mapping_numerics);
    });
}

int gbrl_hip_set_optimizer(gbrl_hip_model *m, const gbrl_hip_optimizer *opt) {
    return guarded([&] {
        if (!m || !opt) throw gbrl::InvalidArgument("null argument");
        m->engine.model.add_optimizer(*opt);
    });
}

int gbrl_hip_get_metadata(const gbrl_hip_model *m, gbrl_hip_metadata *out) {
    if (!m || !out) return GBRL_HIP_E_INVALID;
    *out = m->engine.model.meta;
    return GBRL_HIP_OK;
}
int gbrl_hip_get_bias(const gbrl_hip_model *m, float *out) {
    if (!m || !out) return GBRL_HIP_E_INVALID;
    std::memcpy(out, m->engine.model.bias.data(), sizeof(float) * m->engine.model.bias.size());
    return GBRL_HIP_OK;
}
int gbrl_hip_get_feature_weights(const gbrl_hip_model *m, float *out) {
    if (!m || !out) return GBRL_HIP_E_INVALID;
    std::memcpy(out, m->engine.model.feature_weights.data(), sizeof(float) * m->engine.model.feature_weights.size());
    return GBRL_HIP_OK;
}
int gbrl_hip_get_feature_mapping(const gbrl_hip_model *m, int32_t *fm, uint8_t *mn) {
    if (!m) return GBRL_HIP_E_INVALID;
    const auto &md = m->engine.model;
    if (fm) std::memcpy(fm, md.feature_mapping.data(), sizeof(int32_t) * md.feature_mapping.size());
    if (mn) std::memcpy(mn, md.mapping_numerics.data(), md.mapping_numerics.size());
    return GBRL_HIP_OK;
}
int gbrl_hip_num_optimizers(const gbrl_hip_model *m) { return m ? static_cast<int>(m->engine.model.opts.size()) : 0; }
int gbrl_hip_get_optimizer(const gbrl_hip_model *m, int idx, gbrl_hip_optimizer *out) {
    if (!m || !out || idx < 0 || idx >= static_cast<int>(m->engine.model.opts.size())) return GBRL_HIP_E_INVALID;
    *out = m->engine.model.opts[idx];
    return GBRL_HIP_OK;
}
int gbrl_hip_get_scheduler_lrs(const gbrl_hip_model *m, float *out) {
    if (!m || !out) return GBRL_HIP_E_INVALID;
    const gbrl::Model &md = m->engine.model;
    for (size_t i = 0; i < md.opts.size(); ++i) out[i] = gbrl::scheduler_lr(md.opts[i], md.meta.n_trees);   // gbrl.cpp:527-539
    return GBRL_HIP_OK;
}
const char *gbrl_hip_learner_name(const gbrl_hip_model *m) { return m ? m->engine.model.learner_name.c_str() : ""; }

int gbrl_hip_get_ensemble(const gbrl_hip_model *m, int32_t *tree_indices, int32_t *depths, float *values,
                          int32_t *feature_indices, float *feature_values, float *edge_weights, uint8_t *is_numerics,
                          uint8_t *inequality_directions, char *categorical_values, int32_t *rev_num, int32_t *rev_cat) {
    if (!m) return GBRL_HIP_E_INVALID;
    const gbrl::Model &md = m->engine.model;
    const size_t T = md.meta.n_trees, L = md.meta.n_leaves, S = md.split_rows(), MD = md.meta.max_depth, D = md.meta.output_dim;
    auto cp = [](void *dst, const void *src, size_t bytes) { if (dst && bytes) std::memcpy(dst, src, bytes); };
    cp(tree_indices, md.tree_indices.data(), T * 4);
    cp(depths, md.depths.data(), S * 4);
    cp(values, md.values.data(), L * D * 4);
    cp(feature_indices, md.feature_indices.data(), S * MD * 4);
    cp(feature_values, md.feature_values.data(), S * MD * 4);
    cp(edge_weights, md.edge_weights.data(), L * MD * 4);
    cp(is_numerics, md.is_numerics.data(), S * MD);
    cp(inequality_directions, md.inequality_directions.data(), L * MD);
    cp(categorical_values, md.categorical_values.data(), S * MD * gbrl::kCat);
    cp(rev_num, md.reverse_num.data(), md.reverse_num.size() * 4);
    cp(rev_cat, md.reverse_cat.data(), md.reverse_cat.size() * 4);
    return GBRL_HIP_OK;
}

int gbrl_hip_step(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                  const float *grads, int grads_on_device, int n_samples, int n_num_features, int n_cat_features) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.step(obs, obs_on_device != 0, cat_obs, cat_on_device != 0, grads, grads_on_device != 0, n_samples,
                       n_num_features, n_cat_features);
    });
}

int gbrl_hip_fit(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                 const float *targets, int targets_on_device, int n_samples, int n_num_features, int n_cat_features,
                 int iterations, int shuffle, float *loss_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        const float loss = m->engine.fit(obs, obs_on_device != 0, cat_obs, cat_on_device != 0, targets, targets_on_device != 0, n_samples,
                                         n_num_features, n_cat_features, iterations, shuffle != 0);
        if (loss_out) *loss_out = loss;
    });
}

int gbrl_hip_predict(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                     int n_samples, int n_num_features, int n_cat_features, int start_tree, int stop_tree, float *out,
                     int out_on_device) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.predict(obs, obs_on_device != 0, cat_obs, cat_on_device != 0, n_samples, n_num_features, n_cat_features,
                          start_tree, stop_tree, out, out_on_device != 0);
    });
}

int gbrl_hip_encode_categorical(gbrl_hip_model *m, const char *cat_obs, int cat_on_device, int n_samples, int n_cat_features, int32_t *ids_out,
                                int ids_on_device, uint64_t *dictionary_token) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.encode_categorical(cat_obs, cat_on_device != 0, n_samples, n_cat_features, ids_out, ids_on_device != 0, dictionary_token);
    });
}

int gbrl_hip_predict_encoded(gbrl_hip_model *m, const float *obs, int obs_on_device, const int32_t *cat_ids, int ids_on_device,
                             uint64_t dictionary_token, int n_samples, int n_num_features, int n_cat_features, int start_tree, int stop_tree,
                             float *out, int out_on_device) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.predict_encoded(obs, obs_on_device != 0, cat_ids, ids_on_device != 0, dictionary_token, n_samples, n_num_features, n_cat_features,
                                  start_tree, stop_tree, out, out_on_device != 0);
    });
}

int gbrl_hip_predict_continue(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device, int n_samples,
                              int n_num_features, int n_cat_features, int start_tree, int stop_tree, const float *base, int base_on_device,
                              float *out, int out_on_device) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.predict_continue(obs, obs_on_device != 0, cat_obs, cat_on_device != 0, n_samples, n_num_features, n_cat_features, start_tree,
                                   stop_tree, base, base_on_device != 0, out, out_on_device != 0);
    });
}

int gbrl_hip_predict_continue_encoded(gbrl_hip_model *m, const float *obs, int obs_on_device, const int32_t *cat_ids, int ids_on_device,
                                      uint64_t dictionary_token, int n_samples, int n_num_features, int n_cat_features, int start_tree,
                                      int stop_tree, const float *base, int base_on_device, float *out, int out_on_device) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.predict_continue_encoded(obs, obs_on_device != 0, cat_ids, ids_on_device != 0, dictionary_token, n_samples, n_num_features,
                                           n_cat_features, start_tree, stop_tree, base, base_on_device != 0, out, out_on_device != 0);
    });
}

int gbrl_hip_predict_staged(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device, int n_samples,
                            int n_num_features, int n_cat_features, const int32_t *stops, int n_stops, float *out, int out_on_device) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.predict_staged(obs, obs_on_device != 0, cat_obs, cat_on_device != 0, n_samples, n_num_features, n_cat_features, stops, n_stops, out,
                                 out_on_device != 0);
    });
}

int gbrl_hip_staged_loss(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device, const float *targets,
                         int targets_on_device, int n_samples, int n_num_features, int n_cat_features, const int32_t *stops, int n_stops,
                         double *loss_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.staged_loss(obs, obs_on_device != 0, cat_obs, cat_on_device != 0, targets, targets_on_device != 0, n_samples, n_num_features,
                              n_cat_features, stops, n_stops, loss_out);
    });
}

int gbrl_hip_predict_leaves(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device, int n_samples,
                            int n_num_features, int n_cat_features, int start_tree, int stop_tree, int32_t *out, int out_on_device) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.predict_leaves(obs, obs_on_device != 0, cat_obs, cat_on_device != 0, nullptr, false, nullptr, n_samples, n_num_features, n_cat_features,
                                 start_tree, stop_tree, out, out_on_device != 0);
    });
}

int gbrl_hip_predict_leaves_encoded(gbrl_hip_model *m, const float *obs, int obs_on_device, const int32_t *cat_ids, int ids_on_device,
                                    uint64_t dictionary_token, int n_samples, int n_num_features, int n_cat_features, int start_tree, int stop_tree,
                                    int32_t *out, int out_on_device) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        if (n_cat_features > 0 && cat_ids == nullptr) throw gbrl::InvalidArgument("Cannot call predict without observations!");
        m->engine.predict_leaves(obs, obs_on_device != 0, nullptr, false, cat_ids, ids_on_device != 0, &dictionary_token, n_samples, n_num_features,
                                 n_cat_features, start_tree, stop_tree, out, out_on_device != 0);
    });
}

int gbrl_hip_leaf_counts(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device, int n_samples,
                         int n_num_features, int n_cat_features, int start_tree, int stop_tree, int64_t *out_host) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.leaf_counts(obs, obs_on_device != 0, cat_obs, cat_on_device != 0, nullptr, false, nullptr, n_samples, n_num_features, n_cat_features,
                              start_tree, stop_tree, out_host);
    });
}

int gbrl_hip_leaf_counts_encoded(gbrl_hip_model *m, const float *obs, int obs_on_device, const int32_t *cat_ids, int ids_on_device,
                                 uint64_t dictionary_token, int n_samples, int n_num_features, int n_cat_features, int start_tree, int stop_tree,
                                 int64_t *out_host) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        if (n_cat_features > 0 && cat_ids == nullptr) throw gbrl::InvalidArgument("Cannot call predict without observations!");
        m->engine.leaf_counts(obs, obs_on_device != 0, nullptr, false, cat_ids, ids_on_device != 0, &dictionary_token, n_samples, n_num_features,
                              n_cat_features, start_tree, stop_tree, out_host);
    });
}

int gbrl_hip_refit_leaves(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device, const float *targets,
                          int targets_on_device, int n_samples, int n_num_features, int n_cat_features, int start_tree, int stop_tree, double decay_rate,
                          double *loss_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.refit_leaves(obs, obs_on_device != 0, cat_obs, cat_on_device != 0, targets, targets_on_device != 0, n_samples, n_num_features,
                               n_cat_features, start_tree, stop_tree, decay_rate, loss_out);
    });
}

// ---- prepared data sets: handles are looked up in a registry, so a destroyed (or never created) handle is an argument error, not a dangling read
gbrl_hip_dataset *gbrl_hip_dataset_create(gbrl_hip_model *m, const float *obs, int obs_on_device, int n_samples, int n_num_features) {
    gbrl_hip_dataset *ds = nullptr;
    g_ds_status = guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        std::unique_ptr<gbrl::PreparedDataset> p(m->engine.prepare_dataset(obs, obs_on_device != 0, n_samples, n_num_features));
        ds = new gbrl_hip_dataset{std::move(p)};
        std::lock_guard<std::mutex> lk(ds_registry().mu);
        ds_registry().live.insert(ds);
    });
    return ds;
}
int gbrl_hip_dataset_last_status(void) { return g_ds_status; }

void gbrl_hip_dataset_destroy(gbrl_hip_dataset *ds) {
    if (!ds) return;
    {
        std::lock_guard<std::mutex> lk(ds_registry().mu);
        if (ds_registry().live.erase(ds) == 0) return;   // not (or no longer) a data set of this library
    }
    delete ds;
}

int gbrl_hip_dataset_info(const gbrl_hip_dataset *ds, gbrl_hip_dataset_desc *out) {
    return guarded([&] {
        const gbrl::PreparedDataset &d = live_dataset(ds);
        if (!out) throw gbrl::InvalidArgument("null argument");
        out->n_rows = d.n; out->n_features = d.F; out->n_bins = d.n_bins; out->generator_type = d.generator_type; out->device = d.device;
        out->code_groups = d.code_groups(); out->nbytes = d.nbytes();
    });
}

int gbrl_hip_dataset_thresholds(const gbrl_hip_dataset *ds, float *out) {
    return guarded([&] {
        const gbrl::PreparedDataset &d = live_dataset(ds);
        if (!out) throw gbrl::InvalidArgument("null argument");
        std::memcpy(out, d.h_thr.data(), sizeof(float) * d.h_thr.size());
    });
}

int gbrl_hip_dataset_codes(const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, uint16_t *out) {
    return guarded([&] { live_dataset(ds).codes_to_host(rows, rows_on_device != 0, n_rows, out); });
}

int gbrl_hip_step_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *grads, int grads_on_device, const int32_t *rows,
                           int rows_on_device, int n_rows) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.step_prepared(&live_dataset(ds), grads, grads_on_device != 0, rows, rows_on_device != 0, n_rows);
    });
}

// ---- column subsets of a data set (gather_cols.hip): a step on them, their codes, the column rule on the host, the kernel's geometry
int gbrl_hip_step_prepared_cols(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *grads, int grads_on_device, const int32_t *rows,
                                int rows_on_device, int n_rows, const int32_t *cols, int n_cols) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        if (cols == nullptr) throw gbrl::InvalidArgument("step_prepared: null cols");
        m->engine.step_prepared(&live_dataset(ds), grads, grads_on_device != 0, rows, rows_on_device != 0, n_rows, cols, n_cols);
    });
}

int gbrl_hip_dataset_codes_cols(const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, const int32_t *cols, int n_cols,
                                uint16_t *out) {
    return guarded([&] {
        const gbrl::PreparedDataset &d = live_dataset(ds);
        if (cols == nullptr) throw gbrl::InvalidArgument("dataset_codes: null cols");
        d.codes_to_host(rows, rows_on_device != 0, n_rows, out, cols, n_cols);
    });
}

int gbrl_hip_sample_cols_host(int n_features, double colsample, uint64_t seed, int draw, int32_t *out, int *count) {
    return guarded([&] { gbrl::Engine::sample_cols_host(n_features, colsample, seed, draw, out, count); });
}

void gbrl_hip_gather_cols_geometry(int *rows_per_tile, int *max_staged_groups) {
    if (rows_per_tile) *rows_per_tile = gbrl::kern::kGatherColsRows;
    if (max_staged_groups) *max_staged_groups = gbrl::kern::kGatherColsMaxStaged;
}

// ---- the walk over a data set's bin codes
int gbrl_hip_condition_bins(const gbrl_hip_model *m, const float *thresholds, int n_features, int n_bins, int32_t *out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.condition_bins(thresholds, n_features, n_bins, out);
    });
}

int gbrl_hip_predict_continue_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows,
                                       const float *base, int base_on_device, int start_tree, int stop_tree, float *out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.precheck_prepared("predict_continue_prepared");
        m->engine.predict_continue_prepared(&live_dataset(ds), rows, rows_on_device != 0, n_rows, base, base_on_device != 0, start_tree, stop_tree, out,
                                            base_on_device != 0);
    });
}

// The one body of the eight gbrl_hip_fit_prepared* spellings.  valid_required (gbrl_hip_fit_prepared_valid): a NULL valid_ds is a null data set;
// otherwise it means "no validation", the other validation arguments must then be at their defaults, *iterations_done = iterations and
// *best_n_trees is left alone.  Every refusal that needs no data set comes before a handle is resolved, the validation handle before the
// training handle, and nothing is written on a refusal.
static int fit_prepared_call(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations, bool valid_required,
                             const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds, double min_delta,
                             const gbrl::FitOptions &opt, float *loss_out, double *valid_loss_out, int *iterations_done, int *best_n_trees,
                             double *valid_metric_out = nullptr, const float *valid_weights = nullptr, int valid_weights_on_device = 0,
                             float *weight_max_out = nullptr, const int32_t *valid_group = nullptr, int valid_n_groups = 0) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        gbrl::Engine::FitValid v{nullptr, valid_targets, valid_targets_on_device != 0, early_stopping_rounds, min_delta, valid_loss_out, 0, 0, valid_metric_out,
                                 valid_weights, valid_weights_on_device != 0, valid_group, valid_n_groups};
        gbrl::Engine::FitValid *valid = valid_required || valid_ds != nullptr ? &v : nullptr;
        m->engine.precheck_fit(targets, iterations, opt, valid);
        if (!valid && (valid_group != nullptr || valid_n_groups != 0)) throw gbrl::InvalidArgument("fit_prepared: valid_group needs a validation set (valid=)");
        if (!valid && (valid_targets != nullptr || early_stopping_rounds != 0 || min_delta != 0.0 || valid_loss_out != nullptr || valid_metric_out != nullptr))
            throw gbrl::InvalidArgument("fit_prepared: valid_targets, early_stopping_rounds, min_delta and valid_loss_out need a validation set");
        if (!valid && valid_weights != nullptr) throw gbrl::InvalidArgument("fit_prepared: valid_weights need a validation set (valid=)");
        if (valid) v.ds = &live_dataset(valid_ds);
        float weight_max = 0.0f;
        const float loss = m->engine.fit_prepared(&live_dataset(ds), targets, targets_on_device != 0, iterations, opt, valid, &weight_max);
        if (loss_out) *loss_out = loss;
        if (weight_max_out) *weight_max_out = weight_max;
        if (iterations_done) *iterations_done = valid ? v.done : iterations;
        if (valid && best_n_trees) *best_n_trees = v.best_n_trees;
    });
}

int gbrl_hip_fit_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *targets, int targets_on_device, int iterations, float *loss_out) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, nullptr, nullptr, 0, 0, 0.0, {}, loss_out, nullptr, nullptr, nullptr);
}

// ---- data sets that share thresholds; validation and early stopping
gbrl_hip_dataset *gbrl_hip_dataset_create_like(gbrl_hip_model *m, const gbrl_hip_dataset *reference, const float *obs, int obs_on_device, int n_samples) {
    gbrl_hip_dataset *ds = nullptr;
    g_ds_status = guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.precheck_prepared("prepare_dataset");
        // (the registry lock is not held over the device work: destroying the reference during this call is the caller's race, as for a step)
        std::unique_ptr<gbrl::PreparedDataset> p(m->engine.prepare_dataset_like(&live_dataset(reference), obs, obs_on_device != 0, n_samples));
        ds = new gbrl_hip_dataset{std::move(p)};
        std::lock_guard<std::mutex> lk(ds_registry().mu);
        ds_registry().live.insert(ds);
    });
    return ds;
}

uint64_t gbrl_hip_dataset_thresholds_id(const gbrl_hip_dataset *ds) {
    uint64_t id = 0;
    (void)guarded([&] { id = live_dataset(ds).thresholds_id; });
    return id;
}

int gbrl_hip_fit_prepared_valid(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *targets, int targets_on_device, int iterations,
                                const gbrl_hip_dataset *valid_ds, const float *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                double min_delta, float *loss_out, double *valid_loss_out, int *iterations_done, int *best_n_trees) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, true, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {}, loss_out, valid_loss_out, iterations_done, best_n_trees);
}

int gbrl_hip_early_stop_scan(const double *curve, int n, int rounds, double min_delta, int *stop_after, int *best) {
    return guarded([&] { gbrl::Engine::early_stop_scan(curve, n, rounds, min_delta, stop_after, best); });
}

// ---- row subsampling: the sampler on the host, on a data set's rows, fused with a gather (test helper), and fit_prepared on samples
int gbrl_hip_sample_rows_host(int row0, int n, double subsample, uint64_t seed, int draw, int32_t *out, int *count) {
    return guarded([&] { gbrl::Engine::sample_rows_host(row0, n, subsample, seed, draw, out, count); });
}

int gbrl_hip_dataset_sample_rows(const gbrl_hip_dataset *ds, int row0, int n, double subsample, uint64_t seed, int draw, int32_t *out, int out_on_device,
                                 int *count) {
    return guarded([&] { gbrl::Engine::sample_rows(&live_dataset(ds), row0, n, subsample, seed, draw, out, out_on_device != 0, count); });
}

int gbrl_hip_sample_gather(int row0, int n, double subsample, uint64_t seed, int draw, const float *grads, int output_dim, int32_t *rows_out,
                           float *grads_out, int *count) {
    return guarded([&] { gbrl::Engine::sample_gather(row0, n, subsample, seed, draw, grads, output_dim, rows_out, grads_out, count); });
}

void gbrl_hip_sample_rows_geometry(int *rows_per_block, int *scan_width) {
    if (rows_per_block) *rows_per_block = gbrl::kern::kSampleRowsPerBlock;
    if (scan_width) *scan_width = gbrl::kern::kSampleScanWidth;
}

int gbrl_hip_fit_prepared_sampled(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *targets, int targets_on_device, int iterations,
                                  const gbrl_hip_dataset *valid_ds, const float *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                  double min_delta, double subsample, uint64_t seed, float *loss_out, double *valid_loss_out, int *iterations_done,
                                  int *best_n_trees) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {subsample, 1.0, seed, GBRL_HIP_OBJ_RMSE}, loss_out, valid_loss_out, iterations_done, best_n_trees);
}

int gbrl_hip_fit_prepared_colsampled(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *targets, int targets_on_device, int iterations,
                                     const gbrl_hip_dataset *valid_ds, const float *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                     double min_delta, double subsample, double colsample, uint64_t seed, float *loss_out, double *valid_loss_out,
                                     int *iterations_done, int *best_n_trees) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {subsample, colsample, seed, GBRL_HIP_OBJ_RMSE}, loss_out, valid_loss_out, iterations_done, best_n_trees);
}

// ---- classification objectives: fit_prepared with one, the gradient and loss of a prediction matrix, the gradient rule on the host
static_assert(gbrl::kern::kObjRmse == GBRL_HIP_OBJ_RMSE && gbrl::kern::kObjLogistic == GBRL_HIP_OBJ_LOGISTIC && gbrl::kern::kObjSoftmax == GBRL_HIP_OBJ_SOFTMAX,
              "the kernels' objectives are the header's");
int gbrl_hip_fit_prepared_objective(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                                    const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                    double min_delta, double subsample, double colsample, uint64_t seed, int objective, float *loss_out,
                                    double *valid_loss_out, int *iterations_done, int *best_n_trees) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {subsample, colsample, seed, objective}, loss_out, valid_loss_out, iterations_done, best_n_trees);
}

// ---- classifier metrics: fit_prepared watched by one, the metric of a prediction matrix on the device and on the host
static_assert(gbrl::kern::kMetricNone == GBRL_HIP_METRIC_NONE && gbrl::kern::kMetricError == GBRL_HIP_METRIC_ERROR && gbrl::kern::kMetricAuc == GBRL_HIP_METRIC_AUC,
              "the kernels' metrics are the header's");
int gbrl_hip_fit_prepared_metric(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                                 const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                 double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, float *loss_out,
                                 double *valid_loss_out, double *valid_metric_out, int *iterations_done, int *best_n_trees) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {subsample, colsample, seed, objective, metric}, loss_out, valid_loss_out, iterations_done, best_n_trees, valid_metric_out);
}

// ---- Newton leaf values: fit_prepared with them, one tree's leaves on a data set, the hessian and the value rule on the host
static_assert(gbrl::kern::kLeafGradient == GBRL_HIP_LEAF_GRADIENT && gbrl::kern::kLeafNewton == GBRL_HIP_LEAF_NEWTON, "the kernels' leaf updates are the header's");
int gbrl_hip_fit_prepared_leaf(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                               const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                               double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update, double leaf_l2,
                               float *loss_out, double *valid_loss_out, double *valid_metric_out, int *iterations_done, int *best_n_trees) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {subsample, colsample, seed, objective, metric, leaf_update, leaf_l2}, loss_out, valid_loss_out, iterations_done, best_n_trees,
                             valid_metric_out);
}

// ---- row weights: the weighted spellings; the older ones forward without weights
static_assert(gbrl::kern::kWeightMax == GBRL_HIP_WEIGHT_MAX, "the kernels' largest weight is the header's");
int gbrl_hip_fit_prepared_weighted(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                                   const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                   double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update, double leaf_l2,
                                   const float *weights, int weights_on_device, const float *valid_weights, int valid_weights_on_device, float *loss_out,
                                   double *valid_loss_out, double *valid_metric_out, int *iterations_done, int *best_n_trees, float *weight_max_out) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {subsample, colsample, seed, objective, metric, leaf_update, leaf_l2, weights, weights_on_device != 0}, loss_out, valid_loss_out,
                             iterations_done, best_n_trees, valid_metric_out, valid_weights, valid_weights_on_device, weight_max_out);
}

// ---- one-side sampling: the rule on the host, the device kernels on a data set's rows, fit_prepared with the draw
int gbrl_hip_goss_rows_host(const float *grads, int output_dim, int row0, int n, double top_rate, double other_rate, uint64_t seed, int draw, int32_t *rows_out,
                            float *factor_out, float *grads_out, int *count) {
    return guarded([&] { gbrl::Engine::goss_rows_host(grads, output_dim, row0, n, top_rate, other_rate, seed, draw, rows_out, factor_out, grads_out, count); });
}

int gbrl_hip_dataset_sample_goss(const gbrl_hip_dataset *ds, const float *grads, int output_dim, int row0, int n, double top_rate, double other_rate, uint64_t seed,
                                 int draw, int32_t *rows_out, float *factor_out, float *grads_out, int on_device, int *count, int *n_top, uint32_t *tau_bits) {
    return guarded([&] {
        gbrl::Engine::sample_goss(&live_dataset(ds), grads, output_dim, row0, n, top_rate, other_rate, seed, draw, rows_out, factor_out, grads_out, on_device != 0, count,
                                  n_top, tau_bits);
    });
}

int gbrl_hip_fit_prepared_goss(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                               const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds, double min_delta,
                               double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update, double leaf_l2, const float *weights,
                               int weights_on_device, const float *valid_weights, int valid_weights_on_device, double goss_top, double goss_other, float *loss_out,
                               double *valid_loss_out, double *valid_metric_out, int *iterations_done, int *best_n_trees, float *weight_max_out) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {subsample, colsample, seed, objective, metric, leaf_update, leaf_l2, weights, weights_on_device != 0, goss_top, goss_other}, loss_out,
                             valid_loss_out, iterations_done, best_n_trees, valid_metric_out, valid_weights, valid_weights_on_device, weight_max_out);
}

// ---- quantile regression: fit_prepared with the levels, one tree's leaf quantiles on a data set, the rules on the host
static_assert(gbrl::kern::kObjQuantile == GBRL_HIP_OBJ_QUANTILE && gbrl::kern::kLeafQuantile == GBRL_HIP_LEAF_QUANTILE, "the kernels' quantile codes are the header's");
int gbrl_hip_fit_prepared_quantile(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                                   const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                   double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update, double leaf_l2,
                                   const float *weights, int weights_on_device, const float *valid_weights, int valid_weights_on_device, double goss_top,
                                   double goss_other, const float *alpha, float *loss_out, double *valid_loss_out, double *valid_metric_out, int *iterations_done,
                                   int *best_n_trees, float *weight_max_out) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {subsample, colsample, seed, objective, metric, leaf_update, leaf_l2, weights, weights_on_device != 0, goss_top, goss_other, alpha},
                             loss_out, valid_loss_out, iterations_done, best_n_trees, valid_metric_out, valid_weights, valid_weights_on_device, weight_max_out);
}

int gbrl_hip_quantile_leaves_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, const float *pred,
                                      int pred_on_device, const float *targets, int targets_on_device, const float *alpha, int tree, float *values_out,
                                      int64_t *counts_out, int64_t *ranks_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.precheck_prepared("quantile_leaves_prepared");
        m->engine.quantile_leaves_prepared(&live_dataset(ds), rows, rows_on_device != 0, n_rows, pred, pred_on_device != 0, targets, targets_on_device != 0, alpha, tree,
                                           values_out, counts_out, ranks_out);
    });
}

int gbrl_hip_leaf_quantile_host(const float *x, const int32_t *leaves, int m, int D, int n_leaves, const float *alpha, float *values_out, int64_t *counts_out,
                                int64_t *ranks_out) {
    return guarded([&] { gbrl::Engine::leaf_quantile_host(x, leaves, m, D, n_leaves, alpha, values_out, counts_out, ranks_out); });
}

int gbrl_hip_quantile_rank(int64_t m, float a, int64_t *rank_out) {
    return guarded([&] {
        if (rank_out == nullptr) throw gbrl::InvalidArgument("quantile_rank: null argument");
        *rank_out = gbrl::Engine::quantile_rank(m, a);
    });
}

void gbrl_hip_leaf_quantile_geometry(int *max_select_leaves, int *rows_per_chunk) { gbrl::kern::leaf_quantile_geometry(max_select_leaves, rows_per_chunk); }

// ---- ranking objectives: fit_prepared with query groups, one tree's Newton leaves, the gradient on the device and on the host, the table, the caps
static_assert(gbrl::kern::kObjPairwise == GBRL_HIP_OBJ_PAIRWISE && gbrl::kern::kObjLambdarank == GBRL_HIP_OBJ_LAMBDARANK, "the kernels' ranking codes are the header's");
int gbrl_hip_fit_prepared_rank(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                               const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds, double min_delta,
                               double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update, double leaf_l2, const float *weights,
                               int weights_on_device, const float *valid_weights, int valid_weights_on_device, double goss_top, double goss_other, const float *alpha,
                               const int32_t *group, int n_groups, int ndcg_at, const int32_t *valid_group, int valid_n_groups, float *loss_out,
                               double *valid_loss_out, double *valid_metric_out, int *iterations_done, int *best_n_trees, float *weight_max_out) {
    return fit_prepared_call(m, ds, targets, targets_on_device, iterations, false, valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta,
                             {subsample, colsample, seed, objective, metric, leaf_update, leaf_l2, weights, weights_on_device != 0, goss_top, goss_other, alpha, group,
                              n_groups, ndcg_at},
                             loss_out, valid_loss_out, iterations_done, best_n_trees, valid_metric_out, valid_weights, valid_weights_on_device, weight_max_out, valid_group,
                             valid_n_groups);
}

int gbrl_hip_newton_leaves_prepared_rank(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *pred, int pred_on_device, const int32_t *labels,
                                         int labels_on_device, const int32_t *group, int n_groups, int objective, int ndcg_at, int tree, double leaf_l2,
                                         int64_t *sums_out, int *bits_out, float *values_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.precheck_prepared("newton_leaves_prepared");
        m->engine.newton_leaves_prepared_rank(&live_dataset(ds), pred, pred_on_device != 0, labels, labels_on_device != 0, group, n_groups, objective, ndcg_at, tree,
                                              leaf_l2, sums_out, bits_out, values_out);
    });
}

int gbrl_hip_rank_gradient(gbrl_hip_model *m, const float *pred, int pred_on_device, const int32_t *labels, int labels_on_device, const int32_t *group, int n_groups,
                           int n, int objective, int ndcg_at, float *grad_out, float *hess_out, double *loss_out, double *ndcg_out, int32_t *positions_out,
                           int64_t *pairs_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.rank_gradient(pred, pred_on_device != 0, labels, labels_on_device != 0, group, n_groups, n, objective, ndcg_at, grad_out, hess_out, loss_out,
                                ndcg_out, positions_out, pairs_out);
    });
}

int gbrl_hip_rank_gradient_host(const float *pred, const int32_t *labels, const int32_t *group, int n_groups, int n, int objective, int ndcg_at, float *grad_out,
                                float *hess_out, double *loss_out, double *ndcg_out, int32_t *positions_out, int64_t *pairs_out) {
    return guarded([&] {
        gbrl::Engine::rank_gradient_host(pred, labels, group, n_groups, n, objective, ndcg_at, grad_out, hess_out, loss_out, ndcg_out, positions_out, pairs_out);
    });
}

int gbrl_hip_rank_discounts(double *out) {
    return guarded([&] {
        if (out == nullptr) throw gbrl::InvalidArgument("rank_discounts: null argument");
        std::memcpy(out, gbrl::Engine::rank_discounts(), sizeof(double) * gbrl::kern::kRankMaxQuery);
    });
}

void gbrl_hip_rank_geometry(int *max_query, int *max_label) {
    if (max_query) *max_query = gbrl::kern::kRankMaxQuery;
    if (max_label) *max_label = gbrl::kern::kRankMaxLabel;
}

// ---- feature importance: the permutation rule on the host, the permuted losses of a data set (engine_importance.hip), the two counts (explain.cpp)
int gbrl_hip_permutation_host(int n, uint64_t seed, int col, int repeat, int32_t *out) {
    return guarded([&] { gbrl::Engine::permutation_host(n, seed, col, repeat, out); });
}

int gbrl_hip_permutation_importance_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int objective,
                                             const float *alpha, int n_repeats, uint64_t seed, const int32_t *cols, int n_cols, int n_trees, double *baseline_out,
                                             double *loss_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.precheck_prepared("permutation_importance_prepared");
        m->engine.permutation_importance_prepared(&live_dataset(ds), targets, targets_on_device != 0, objective, alpha, n_repeats, seed, cols, n_cols, n_trees,
                                                  baseline_out, loss_out);
    });
}

void gbrl_hip_permutation_geometry(int *launch_variants, int *tile_rows) {
    if (launch_variants) *launch_variants = gbrl::kern::kPermLaunchVariants;
    if (tile_rows) *tile_rows = gbrl::kern::perm_tile_rows();
}

// ---- partial dependence: the break rule on the host, the variants' sums and ICE rows of a data set (engine_pd.hip; pd_core.h has the plan)
int gbrl_hip_partial_dependence_codes(const gbrl_hip_model *m, const float *thresholds, int n_features, int n_bins, int col, int n_trees, int32_t *out, int *count) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.partial_dependence_codes(thresholds, n_features, n_bins, col, n_trees, out, count);
    });
}

int gbrl_hip_partial_dependence_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *variants, int n_variants, const int32_t *rows, int rows_on_device,
                                         int n_rows, int n_trees, double *sums_out, float *ice_out, int ice_on_device) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.precheck_prepared("partial_dependence_prepared");
        m->engine.partial_dependence_prepared(&live_dataset(ds), variants, n_variants, rows, rows_on_device != 0, n_rows, n_trees, sums_out, ice_out, ice_on_device != 0);
    });
}

int gbrl_hip_partial_dependence_cells(int col0, const int32_t *codes0, int n0, int col1, const int32_t *codes1, int n1, int32_t *out) {
    return guarded([&] {
        if (codes0 == nullptr || out == nullptr || n0 < 1 || col0 < 0) throw gbrl::InvalidArgument("partial_dependence_cells: a column >= 0, its codes and a place for the cells are needed");
        if (col1 >= 0 && (codes1 == nullptr || n1 < 1)) throw gbrl::InvalidArgument("partial_dependence_cells: the second column has no codes");
        if (col1 >= 0 && col1 == col0) throw gbrl::InvalidArgument("partial_dependence_cells: a pair needs two distinct columns");
        std::vector<gbrl::kern::PdVariant> cells;
        cells.reserve(static_cast<size_t>(gbrl::kern::pd_cell_count(n0, col1 < 0 ? 0 : n1)));
        gbrl::kern::pd_append_cells(cells, col0, codes0, n0, col1 < 0 ? -1 : col1, codes1, col1 < 0 ? 0 : n1);
        static_assert(sizeof(gbrl::kern::PdVariant) == 4 * sizeof(int32_t), "a variant is four int32");
        std::memcpy(out, cells.data(), cells.size() * sizeof(gbrl::kern::PdVariant));
    });
}

void gbrl_hip_partial_dependence_geometry(int n_rows, int output_dim, int *rows_per_partial, int *launch_variants, int *max_launch_variants, uint64_t *scratch_budget_bytes) {
    if (rows_per_partial) *rows_per_partial = gbrl::kern::kPdPartialRows;
    if (launch_variants) *launch_variants = gbrl::kern::pd_launch_variants(n_rows < 1 ? 1 : n_rows, output_dim);
    if (max_launch_variants) *max_launch_variants = gbrl::kern::kPdMaxLaunchVariants;
    if (scratch_budget_bytes) *scratch_budget_bytes = gbrl::kern::kPdScratchBudget;
}

// ---- SHAP values on a data set: the matrix, its column sums, the reduction rule on the host (engine_explain.hip; shap_core.h has the rule and the plan)
int gbrl_hip_shap_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, int tree_idx,
                           const float *norm_values, const float *base_poly, const float *offset, float *out, int out_on_device) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.precheck_prepared("shap_prepared");
        m->engine.shap_prepared(&live_dataset(ds), rows, rows_on_device != 0, n_rows, tree_idx, norm_values, base_poly, offset, out, out_on_device != 0);
    });
}

int gbrl_hip_shap_importance_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows,
                                      const float *norm_values, const float *base_poly, const float *offset, int chunk_rows, double *sum_out, double *abs_out,
                                      int *chunk_rows_used) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.precheck_prepared("shap_importance_prepared");
        m->engine.shap_importance_prepared(&live_dataset(ds), rows, rows_on_device != 0, n_rows, norm_values, base_poly, offset, chunk_rows, sum_out, abs_out,
                                           chunk_rows_used);
    });
}

int gbrl_hip_shap_sums_host(const float *phi, int64_t n_rows, int64_t n_cols, double *sum_out, double *abs_out) {
    return guarded([&] {
        if (sum_out == nullptr || abs_out == nullptr || n_rows < 0 || n_cols < 0 || (phi == nullptr && n_rows > 0 && n_cols > 0))
            throw gbrl::InvalidArgument("shap_sums_host: a matrix [n_rows][n_cols] and a place for the two sums are needed");
        gbrl::kern::shap_sums_host(phi, n_rows, static_cast<size_t>(n_cols), sum_out, abs_out);
    });
}

void gbrl_hip_shap_geometry(int n_features, int output_dim, int *tile_rows, int *default_chunk_rows, uint64_t *budget_bytes) {
    if (tile_rows) *tile_rows = gbrl::kern::kShapTileRows;
    if (default_chunk_rows) *default_chunk_rows = gbrl::kern::shap_default_chunk_rows(n_features, output_dim);
    if (budget_bytes) *budget_bytes = gbrl::kern::kShapScratchBudget;
}

static_assert(GBRL_HIP_IMPORTANCE_SPLIT == gbrl::kFeatureSplit && GBRL_HIP_IMPORTANCE_COVER == gbrl::kFeatureCover, "the importance kinds are the header's");
int gbrl_hip_feature_importance(const gbrl_hip_model *m, int kind, const int64_t *leaf_counts, double *out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        gbrl::feature_importance(m->engine.model, kind, leaf_counts, out);
    });
}

int gbrl_hip_objective_gradient_quantile(gbrl_hip_model *m,const float *pred, int pred_on_device, const void *targets, int targets_on_device, const float *alpha,
                                         int n, int objective, float *grad_out, double *loss_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.objective_gradient(pred, pred_on_device != 0, targets, targets_on_device != 0, n, objective, grad_out, loss_out, nullptr, false, alpha);
    });
}

int gbrl_hip_objective_gradient_host_quantile(const float *pred, const void *targets, const float *alpha, int n, int D, int objective, float *grad_out) {
    return guarded([&] { gbrl::Engine::objective_gradient_host(pred, targets, n, D, objective, grad_out, nullptr, alpha); });
}

int gbrl_hip_newton_leaves_prepared_weighted(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, const float *pred,
                                             int pred_on_device, const void *targets, int targets_on_device, int objective, int tree, double leaf_l2,
                                             const float *weights, int weights_on_device, float weight_max, int64_t *sums_out, int *bits_out, float *values_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.precheck_prepared("newton_leaves_prepared");
        m->engine.newton_leaves_prepared(&live_dataset(ds), rows, rows_on_device != 0, n_rows, pred, pred_on_device != 0, targets, targets_on_device != 0, objective,
                                         tree, leaf_l2, sums_out, bits_out, values_out, weights, weights_on_device != 0, weight_max);
    });
}

int gbrl_hip_newton_leaves_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, const float *pred,
                                    int pred_on_device, const void *targets, int targets_on_device, int objective, int tree, double leaf_l2, int64_t *sums_out,
                                    int *bits_out, float *values_out) {
    return gbrl_hip_newton_leaves_prepared_weighted(m, ds, rows, rows_on_device, n_rows, pred, pred_on_device, targets, targets_on_device, objective, tree, leaf_l2,
                                                    nullptr, 0, -1.0f, sums_out, bits_out, values_out);
}

int gbrl_hip_objective_hessian_host_weighted(const float *pred, const float *weights, int n, int D, int objective, float *hess_out) {
    return guarded([&] { gbrl::Engine::objective_hessian_host(pred, n, D, objective, hess_out, weights); });
}

int gbrl_hip_objective_hessian_host(const float *pred, int n, int D, int objective, float *hess_out) {
    return gbrl_hip_objective_hessian_host_weighted(pred, nullptr, n, D, objective, hess_out);
}

int gbrl_hip_newton_sum_bits_weighted(int64_t m, float weight_max) {
    int bits = 0;
    const int rc = guarded([&] {
        if (gbrl::kern::obj_weight_bad(weight_max))
            throw gbrl::InvalidArgument("newton_sum_bits: weight_max must be a finite number in [0, 65536], got " + std::to_string(weight_max));
        bits = gbrl::kern::newton_sum_bits(static_cast<long long>(m), weight_max);
    });
    return rc == GBRL_HIP_OK ? bits : rc;
}

int gbrl_hip_newton_values_host(const int64_t *sums, int n_leaves, int D, int bits, const float *old_values, const int32_t *depths, double leaf_l2,
                                float *values_out) {
    return guarded([&] { gbrl::Engine::newton_values_host(sums, n_leaves, D, bits, old_values, depths, leaf_l2, values_out); });
}

int gbrl_hip_newton_sum_bits(int64_t m) { return gbrl::kern::newton_sum_bits(static_cast<long long>(m)); }

int gbrl_hip_eval_metric(gbrl_hip_model *m, const float *pred, int pred_on_device, const void *targets, int targets_on_device, int n, int objective, int metric,
                         double *value_out, int64_t *counts_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.eval_metric(pred, pred_on_device != 0, targets, targets_on_device != 0, n, objective, metric, value_out, counts_out);
    });
}

int gbrl_hip_eval_metric_host(const float *pred, const void *targets, int n, int D, int objective, int metric, double *value_out, int64_t *counts_out) {
    return guarded([&] { gbrl::Engine::eval_metric_host(pred, targets, n, D, objective, metric, value_out, counts_out); });
}

int gbrl_hip_objective_gradient_weighted(gbrl_hip_model *m, const float *pred, int pred_on_device, const void *targets, int targets_on_device, const float *weights,
                                         int weights_on_device, int n, int objective, float *grad_out, double *loss_out) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.objective_gradient(pred, pred_on_device != 0, targets, targets_on_device != 0, n, objective, grad_out, loss_out, weights, weights_on_device != 0);
    });
}

int gbrl_hip_objective_gradient(gbrl_hip_model *m, const float *pred, int pred_on_device, const void *targets, int targets_on_device, int n, int objective,
                                float *grad_out, double *loss_out) {
    return gbrl_hip_objective_gradient_weighted(m, pred, pred_on_device, targets, targets_on_device, nullptr, 0, n, objective, grad_out, loss_out);
}

int gbrl_hip_objective_gradient_host_weighted(const float *pred, const void *targets, const float *weights, int n, int D, int objective, float *grad_out) {
    return guarded([&] { gbrl::Engine::objective_gradient_host(pred, targets, n, D, objective, grad_out, weights); });
}

int gbrl_hip_objective_gradient_host(const float *pred, const void *targets, int n, int D, int objective, float *grad_out) {
    return gbrl_hip_objective_gradient_host_weighted(pred, targets, nullptr, n, D, objective, grad_out);
}

int gbrl_hip_objective_exp_host(const float *t, int n, double *out, float *out_f32) {
    return guarded([&] {
        if (t == nullptr || (out == nullptr && out_f32 == nullptr)) throw gbrl::InvalidArgument("objective_exp_host: null argument");
        if (n < 0) throw gbrl::InvalidArgument("objective_exp_host: n must be >= 0");
        for (int i = 0; i < n; ++i) {
            if (out) out[i] = gbrl::kern::obj_exp(t[i]);
            if (out_f32) out_f32[i] = gbrl::kern::obj_exp_f32(t[i]);
        }
    });
}

int gbrl_hip_leaf_counts_chunk(void) { return gbrl::kern::leaf_counts_chunk(); }

static_assert(static_cast<int>(gbrl::Engine::ParityMode::Default) == GBRL_HIP_PARITY_DEFAULT && static_cast<int>(gbrl::Engine::ParityMode::Reference) == GBRL_HIP_PARITY_REFERENCE &&
              static_cast<int>(gbrl::Engine::ParityMode::ExactArgmax) == GBRL_HIP_PARITY_EXACT_ARGMAX, "the engine's parity modes are the header's");
int gbrl_hip_set_parity_mode(gbrl_hip_model *m, int mode, int max_node_rows) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        if (mode != GBRL_HIP_PARITY_DEFAULT && mode != GBRL_HIP_PARITY_REFERENCE && mode != GBRL_HIP_PARITY_EXACT_ARGMAX)
            throw gbrl::InvalidArgument("Invalid parity mode! Options are: default/reference/exact_argmax");
        m->engine.set_parity(static_cast<gbrl::Engine::ParityMode>(mode), max_node_rows);
    });
}
int gbrl_hip_get_parity_mode(const gbrl_hip_model *m, int *mode, int *max_node_rows) {
    if (!m) return GBRL_HIP_E_INVALID;
    const gbrl::Engine::Parity p = m->engine.parity();
    if (mode) *mode = static_cast<int>(p.mode);
    if (max_node_rows) *max_node_rows = p.max_node_rows;
    return GBRL_HIP_OK;
}

int gbrl_hip_set_collective(gbrl_hip_model *m, const gbrl_hip_collective *hooks) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.set_collective(hooks);
    });
}

int gbrl_hip_rccl_available(void) { return gbrl::rccl_api().ok ? 1 : 0; }
int gbrl_hip_rccl_unique_id(void *id128) {
    return guarded([&] {
        if (!id128) throw gbrl::InvalidArgument("null id buffer");
        const gbrl::RcclApi &api = gbrl::rccl_api();
        if (!api.ok) throw gbrl::Unsupported("RCCL is not available in this process");
        gbrl::RcclApi::UniqueId id;
        if (api.GetUniqueId(&id) != 0) throw gbrl::HipError("ncclGetUniqueId failed");
        std::memcpy(id128, id.internal, sizeof(id.internal));
    });
}
int gbrl_hip_set_rccl(gbrl_hip_model *m, const void *id128, int world_size, int rank) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        m->engine.set_rccl(id128, world_size, rank);
    });
}

int gbrl_hip_set_rccl_flags(gbrl_hip_model *m, const void *id128, int world_size, int rank, unsigned flags) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null model");
        if (flags & ~static_cast<unsigned>(GBRL_HIP_RCCL_KEEP_WORLD1)) throw gbrl::InvalidArgument("unknown RCCL flags");
        m->engine.set_rccl(id128, world_size, rank, (flags & GBRL_HIP_RCCL_KEEP_WORLD1) != 0);
    });
}

// ---- inspection (explain.cpp), served from the host copy of the ensemble ----
int gbrl_hip_tree_shap(const gbrl_hip_model *m, int tree_idx, const float *obs, const char *cat_obs, int n_samples,
                       const float *norm_values, const float *base_poly, const float *offset, float *out) {
    return guarded([&] {
        if (!m || !out || n_samples < 0) throw gbrl::InvalidArgument("null argument");
        const gbrl::Model &md = m->engine.model;
        gbrl::check_shap_arguments(md, tree_idx, obs, cat_obs, norm_values, base_poly, offset);   // validate BEFORE anything is written
        std::memset(out, 0, sizeof(float) * static_cast<size_t>(n_samples) * (md.meta.n_num_features + md.meta.n_cat_features) * md.meta.output_dim);
        // the device evaluates the same recursion with the same roundings (shap.hip); the host copy serves a machine without a GPU
        if (const_cast<gbrl_hip_model *>(m)->engine.shap_on_device(tree_idx, obs, cat_obs, n_samples, norm_values, base_poly, offset, out)) return;
        gbrl::tree_shap(md, tree_idx, obs, cat_obs, n_samples, norm_values, base_poly, offset, out);
    });
}
int gbrl_hip_ensemble_shap(const gbrl_hip_model *m, const float *obs, const char *cat_obs, int n_samples,
                           const float *norm_values, const float *base_poly, const float *offset, float *out) {
    return guarded([&] {
        if (!m || !out || n_samples < 0) throw gbrl::InvalidArgument("null argument");
        const gbrl::Model &md = m->engine.model;
        if (md.meta.n_trees == 0) return;   // nothing to explain; the caller's buffer is sized from its inputs (binding zero-fills)
        gbrl::check_shap_arguments(md, 0, obs, cat_obs, norm_values, base_poly, offset);
        std::memset(out, 0, sizeof(float) * static_cast<size_t>(n_samples) * (md.meta.n_num_features + md.meta.n_cat_features) * md.meta.output_dim);
        if (const_cast<gbrl_hip_model *>(m)->engine.shap_on_device(-1, obs, cat_obs, n_samples, norm_values, base_poly, offset, out)) return;
        gbrl::ensemble_shap(md, obs, cat_obs, n_samples, norm_values, base_poly, offset, out);
    });
}
int gbrl_hip_export(const gbrl_hip_model *m, const char *filename, const char *modelname, const char *export_format,
                    const char *export_type, const char *prefix) {
    bool io_error = false;
    const int rc = guarded([&] {
        if (!m || !filename) throw gbrl::InvalidArgument("null argument");
        // the reference opens (and truncates) the file before it validates anything (gbrl.cpp:1107-1118)
        FILE *f = std::fopen(filename, "wb");
        if (!f) { io_error = true; throw std::runtime_error("File opening error"); }
        std::string text;
        try {
            gbrl::export_header(m->engine.model, modelname ? modelname : "", export_format ? export_format : "float",
                                export_type ? export_type : "full", prefix ? prefix : "", text);
        } catch (...) { std::fclose(f); throw; }
        const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
        if (std::fclose(f) != 0 || !ok) { io_error = true; throw std::runtime_error("Writing to file error"); }
    });
    return (rc != GBRL_HIP_OK && io_error) ? GBRL_HIP_E_IO : rc;
}
int gbrl_hip_print_tree(const gbrl_hip_model *m, int tree_idx) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null argument");
        const std::string t = gbrl::tree_text(m->engine.model, tree_idx);
        std::fwrite(t.data(), 1, t.size(), stdout);
        std::fflush(stdout);
    });
}
int gbrl_hip_print_ensemble_metadata(const gbrl_hip_model *m, const char *device_name) {
    return guarded([&] {
        if (!m) throw gbrl::InvalidArgument("null argument");
        const std::string t = gbrl::metadata_text(m->engine.model, device_name ? device_name : "cuda");
        std::fwrite(t.data(), 1, t.size(), stdout);
        std::fflush(stdout);
    });
}
int gbrl_hip_plot_tree(const gbrl_hip_model *, int, const char *) {
    return guarded([&] { throw gbrl::Unsupported("GBRL compiled without Graphviz! Cannot plot model"); });
}
size_t gbrl_hip_alloc_data_size(const gbrl_hip_model *m) { return m ? gbrl::reference_alloc_bytes(m->engine.model, true) : 0; }

int gbrl_hip_last_phase_times(const gbrl_hip_model *m, const char **names, float *ms, int cap) {
    if (!m) return 0;
    const auto &ph = m->engine.phase_times();
    const int n = static_cast<int>(ph.size());
    for (int i = 0; i < n && i < cap; ++i) {
        if (names) names[i] = ph[i].first.c_str();
        if (ms) ms[i] = ph[i].second;
    }
    return n;
}

int gbrl_hip_replay_scores(const float *grads, const uint8_t *in_node, const uint8_t *goes_right, int n_rows, int output_dim,
                           const float *meanden, int cosine, int min_data_in_leaf, float *out_scores) {
    if (!grads || !in_node || !goes_right || !out_scores || n_rows < 1 || output_dim < 1) return GBRL_HIP_E_INVALID;
    return guarded([&] {
        if (!gbrl::kern::near_tie_selftest(grads, in_node, goes_right, n_rows, output_dim, meanden, cosine != 0, min_data_in_leaf, out_scores))
            throw gbrl::Unsupported("near-tie replay: shape not supported (n_rows <= 65536, output_dim <= 1024) or no HIP device");
    });
}

int gbrl_hip_seq_sums(const float *x, const uint32_t *lens, const float *starts, int n_chains, float *out, uint32_t *n_slow_blocks) {
    if (!lens || !out || n_chains < 0) return GBRL_HIP_E_INVALID;
    return guarded([&] {
        if (!gbrl::kern::seq_sums_selftest(x, lens, starts, n_chains, out, n_slow_blocks)) throw gbrl::HipError("sequential-sum kernels failed (no HIP device?)");
    });
}

int gbrl_hip_seq_sums_model(const float *x, const uint32_t *lens, const float *starts, int n_chains, float *out, uint32_t *n_slow_blocks, uint32_t *n_fast_blocks) {
    if (!lens || !out || n_chains < 0) return GBRL_HIP_E_INVALID;
    return guarded([&] { (void)gbrl::kern::seq_sums_model(x, lens, starts, n_chains, out, n_slow_blocks, n_fast_blocks); });
}

int gbrl_hip_shap_plan(int max_depth, int output_dim, int *threads, int *samples_per_block) {
    if (!threads || !samples_per_block || output_dim < 1) return GBRL_HIP_E_INVALID;
    const int nt = gbrl::kern::shap_block_threads(max_depth, output_dim);
    *threads = nt;
    *samples_per_block = nt > 0 ? nt / output_dim : 0;
    return GBRL_HIP_OK;
}

int gbrl_hip_hist_plan(int n_classes, int output_dim, int n_rows, int fg_in, gbrl_hip_hist_plan_t *plan) {
    if (!plan || n_classes < 1 || n_classes > 65535 || output_dim < 1 || n_rows < 1 || fg_in < 0 || fg_in > 16 || (fg_in & (fg_in - 1)) != 0) return GBRL_HIP_E_INVALID;
    return guarded([&] {
        const int FG = fg_in ? fg_in : gbrl::kern::hist_feature_group(n_classes, output_dim);
        const gbrl::kern::HistPlan r = gbrl::kern::hist_plan(output_dim, FG, n_rows);
        plan->fg = FG; plan->kind = r.kind; plan->param = r.param; plan->pipe = r.pipe; plan->direct_ok = r.direct_ok; plan->countless_ok = r.countless_ok;
        plan->hist_lds_bytes = gbrl::kern::hist_lds_bytes(n_classes, output_dim, FG);
    });
}

int gbrl_hip_hist_probe(gbrl_hip_hist_probe_t *a) {
    if (!a) return GBRL_HIP_E_INVALID;
    return guarded([&] {
        gbrl::kern::HistProbe p{a->codes, a->qg, a->rows, a->chunks, a->root_le, a->slot_map, a->hist, a->hist_elems, a->root_n, a->n_rows, a->output_dim, a->m, a->n_chunks,
                                a->n_nodes, a->n_feature_slots, a->fg, a->n_classes, a->mode, a->count_rows, a->root_F, a->root_B, a->chunks_per_slot, a->scatter_fs, 0, 0, 0, 0, 0};
        const char *why = "";
        const int rc = gbrl::kern::hist_selftest(p, &why);
        if (rc == gbrl::kern::kHistProbeInvalid) throw gbrl::InvalidArgument(why);
        if (rc != gbrl::kern::kHistProbeOk) throw gbrl::HipError("histogram kernels failed (no HIP device?)");
        a->kind = p.kind; a->param = p.param; a->pipe = p.pipe; a->counted = p.counted; a->wrote_direct = p.direct;
    });
}

int gbrl_hip_score_probe(gbrl_hip_score_probe_t *a) {
    if (!a) return GBRL_HIP_E_INVALID;
    return guarded([&] {
        const char *why = "";
        const int rc = gbrl::kern::score_selftest(*a, &why);
        if (rc == gbrl::kern::kHistProbeInvalid) throw gbrl::InvalidArgument(why);
        if (rc != gbrl::kern::kHistProbeOk) throw gbrl::HipError("score kernels failed (no HIP device?)");
    });
}

int gbrl_hip_rows_probe(gbrl_hip_rows_probe_t *a) {
    if (!a) return GBRL_HIP_E_INVALID;
    return guarded([&] {
        const char *why = "";
        const int rc = gbrl::kern::rows_selftest(*a, &why);
        if (rc == gbrl::kern::kHistProbeInvalid) throw gbrl::InvalidArgument(why);
        if (rc != gbrl::kern::kHistProbeOk) throw gbrl::HipError("row kernels failed (no HIP device?)");
    });
}

int gbrl_hip_cat_rank_stats(const char *cells, int n, int n_cat, const float *grads, int output_dim, int cap, int32_t *feature,
                            int32_t *first_row, int32_t *count, float *total, int *n_distinct) {
    if (!cells || !grads || !feature || !first_row || !count || !total || !n_distinct || n < 1 || n_cat < 1 || output_dim < 1 || cap < 1) return GBRL_HIP_E_INVALID;
    *n_distinct = -1;
    return guarded([&] {
        const int rc = gbrl::kern::cat_rank_selftest(cells, n, n_cat, grads, output_dim, cap, feature, first_row, count, total);
        if (rc == -2) throw gbrl::InvalidArgument("cat_rank_stats: more distinct cells than cap");
        if (rc < 0) throw gbrl::HipError("categorical ranking kernels failed (no HIP device, or more than 2^21 distinct cells?)");
        *n_distinct = rc;
    });
}

int gbrl_hip_set_profiling(gbrl_hip_model *m, int enabled) {
    if (!m) return GBRL_HIP_E_INVALID;
    m->engine.set_profiling(enabled < 0 ? 0 : (enabled > 2 ? 2 : enabled));
    return GBRL_HIP_OK;
}

}  // extern "C"
