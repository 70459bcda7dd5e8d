// Host plumbing shared by the encoder objects behind the C ABI (vit.cpp, resnet.cpp, convnext.cpp, swin.cpp, clip_resnet.cpp):
// per-kind launch timing, the config size hand-over, the forward argument check, the centre-crop offset and, for the
// convolutional and Swin engines, the parameter store (padded parameters included), the {weight, bias} record of a convolution
// and the bodies of ap_<who>_set_param / ap_<who>_finalize.  Host C++ only; no kernel source includes it.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "ap_common.h"

namespace ap {

// ---- optional per-launch HIP-event timing (ap_*_profile_enable / ap_*_profile_read): kind -> events of the last forwards
struct LaunchProfiler {
    bool on = false;
    std::vector<hipEvent_t> pool;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> used;
    size_t next = 0;

    LaunchProfiler() = default;
    LaunchProfiler(const LaunchProfiler&) = delete;
    LaunchProfiler& operator=(const LaunchProfiler&) = delete;
    ~LaunchProfiler() {
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
    hipEvent_t next_event() {
        if (next == pool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            pool.push_back(e);
        }
        return pool[next++];
    }
};

// the bodies of ap_<who>_profile_enable / ap_<who>_profile_read (p: the engine's profiler, null for a null handle)
inline int profile_enable(LaunchProfiler* p, const char* who, int on) {
    AP_REQUIRE(p, "%s_profile_enable: null handle", who);
    p->on = on != 0;
    p->used.clear();
    p->next = 0;
    return AP_OK;
}

inline int profile_read(LaunchProfiler* p, const char* who, int engine_kinds, double* ms_by_kind, long long* launches_by_kind,
                        int kinds) {
    AP_REQUIRE(p && ms_by_kind && launches_by_kind && kinds >= engine_kinds, "%s_profile_read: bad arguments", who);
    for (int k = 0; k < kinds; ++k) { ms_by_kind[k] = 0.0; launches_by_kind[k] = 0; }
    for (auto& u : p->used) {
        AP_HIP_CHECK(hipEventSynchronize(u.second.second));
        float ms = 0.f;
        AP_HIP_CHECK(hipEventElapsedTime(&ms, u.second.first, u.second.second));
        ms_by_kind[u.first] += ms;
        launches_by_kind[u.first] += 1;
    }
    p->used.clear();
    p->next = 0;
    return AP_OK;
}

struct ScopedTimer {      // records start/stop events around one launch (group) when profiling is on
    LaunchProfiler& p; int kind; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(LaunchProfiler& p_, int kind_, hipStream_t s_) : p(p_), kind(kind_), s(s_) {
        if (p.on) { a = p.next_event(); b = p.next_event(); if (a) (void)hipEventRecord(a, s); }
    }
    ~ScopedTimer() {
        if (p.on && a && b) { (void)hipEventRecord(b, s); p.used.push_back({kind, {a, b}}); }
    }
};

// ---- config hand-over (ABI v20): struct_size first, fields only ever appended
// ap_<who>_config_init: zero-fill sizeof_caller bytes and record the size
template <class Config>
int config_init(const char* who, Config* cfg, size_t sizeof_caller, size_t v20_size) {
    AP_REQUIRE(cfg, "%s_config_init: null argument", who);
    AP_REQUIRE(sizeof_caller >= v20_size && sizeof_caller % 4 == 0 && sizeof_caller <= 4096,
               "%s_config_init: %zu is not the size of an ap_%s_config (ABI v20: %zu bytes, this library: %zu)", who, sizeof_caller,
               who, v20_size, sizeof(Config));
    memset(cfg, 0, sizeof_caller);
    cfg->struct_size = (uint32_t)sizeof_caller;
    return AP_OK;
}

// ap_<who>_create: never read a byte the caller did not declare, and take only sizes this structure has had.  A size past this
// library's -- a multiple of 4, at most 4096 and at most newer_window bytes past -- is a binding generated from a newer header:
// AP_ERR_UNSUPPORTED.  Every other size is AP_ERR_INVALID, with `hint` appended to the message.  On success *out holds the
// caller's structure (a missing tail zero).
template <class Config>
int accept_config(const char* who, const Config* cfg, size_t newer_window, const char* hint, Config* out) {
    const size_t given = cfg->struct_size, have = sizeof(Config);
    if (given > have && given % 4 == 0 && given <= 4096 && given - have <= newer_window) {
        set_error("%s_create: cfg->struct_size = %zu is larger than this library's ap_%s_config (%zu bytes, ABI %d): the binding "
                  "was generated from a newer include/atlaspatch_hip.h than the library was built from", who, given, who, have,
                  AP_ABI_VERSION);
        return AP_ERR_UNSUPPORTED;
    }
    AP_REQUIRE(given == have,
               "%s_create: cfg->struct_size = %zu is not a size ap_%s_config has had (ABI v20: %zu bytes; this library: %zu): fill "
               "the structure with ap_%s_config_init(&cfg, sizeof cfg)%s", who, given, who, have, have, who, hint);
    memset(out, 0, sizeof(Config));
    memcpy(out, cfg, given < sizeof(Config) ? given : sizeof(Config));
    out->struct_size = (uint32_t)sizeof(Config);
    return AP_OK;
}

// ---- ap_<who>_forward_*: handle, finalize, batch, buffers (`buffers`: the caller's inputs and outputs are all set),
// workspace alignment and size (`need`: ap_<who>_workspace_bytes)
template <class Engine>
int check_forward_args(const char* who, const Engine* m, int n, bool buffers, const void* ws, size_t ws_bytes,
                       size_t (*need)(const Engine*, int)) {
    AP_REQUIRE(m != nullptr, "%s: null handle", who);
    if (!m->finalized) { set_error("%s: ap_%s_finalize has not been called", who, who); return AP_ERR_STATE; }
    AP_REQUIRE(n >= 0, "%s: negative batch", who);
    if (n == 0) return AP_OK;
    AP_REQUIRE(buffers && ws, "%s: null buffer", who);
    AP_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    const size_t required = need(m, n);
    if (ws_bytes < required) {
        set_error("%s: workspace %zu bytes < required %zu", who, ws_bytes, required);
        return AP_ERR_WORKSPACE;
    }
    return AP_OK;
}

// torchvision CenterCrop: top = int(round((full - size) / 2.0)), Python's round (half to even)
inline int center_crop_offset(int full, int size) {
    const int d = full - size;
    return (d / 2) + ((d & 1) && ((d / 2) & 1) ? 1 : 0);
}

// ---- parameter store of the convolutional engines: one device buffer per checkpoint tensor, addressed by its full name
enum ParamKind { P_CONV_W, P_DW_W, P_VEC };

struct DevParam {
    ParamKind kind = P_VEC;
    int cout = 0, cin = 0, cin_stored = 0, ks = 0;   // P_CONV_W: torch [cout, cin, ks, ks]; P_DW_W: [cout, 1, 7, 7]; P_VEC: [cout]
    int cout_stored = 0;        // rows of the device buffer: cout, or more (add_padded: zero weight rows, zero bias behind cout)
    void* d = nullptr;          // P_CONV_W: T [cout_stored][ks][ks][cin_stored]; P_DW_W: f32 [49][cout]; P_VEC: f32 [cout_stored]
    bool set = false;
    size_t torch_count() const { return kind == P_VEC ? (size_t)cout : (size_t)cout * cin * ks * ks; }
};

class ParamStore {
  public:
    int dtype = AP_F32;         // the compute type of the P_CONV_W buffers

    ParamStore() = default;
    ParamStore(const ParamStore&) = delete;
    ParamStore& operator=(const ParamStore&) = delete;
    ~ParamStore() {
        for (auto& kv : params_)
            if (kv.second.d) (void)hipFree(kv.second.d);
    }

    // a zeroed device buffer for `name`; *out stays valid for the store's lifetime (std::map nodes are stable)
    int add(const std::string& name, ParamKind kind, int cout, int cin, int ks, DevParam** out) {
        return add_padded(name, kind, cout, cin, ks, cout, kind == P_CONV_W ? (int)align_up(cin, 8) : cin, out);
    }

    // the same with the stored channel counts given (P_CONV_W: cout_stored >= cout rows of cin_stored >= cin channels, P_VEC:
    // cout_stored >= cout values): what lies behind the checkpoint's channels stays zero, so a padded output channel is exactly
    // bias 0 + 0 and a padded input channel contributes nothing.  The caller still uploads the checkpoint's own shape.
    int add_padded(const std::string& name, ParamKind kind, int cout, int cin, int ks, int cout_stored, int cin_stored,
                   DevParam** out) {
        AP_REQUIRE(kind != P_DW_W || cout_stored == cout, "parameter %s: a depthwise weight cannot be padded", name.c_str());
        AP_REQUIRE(cout_stored >= cout && cin_stored >= cin && (kind != P_CONV_W || cin_stored % 8 == 0),
                   "parameter %s: stored shape %d x %d smaller than %d x %d", name.c_str(), cout_stored, cin_stored, cout, cin);
        DevParam p;
        p.kind = kind; p.cout = cout; p.cin = cin; p.ks = ks;
        p.cout_stored = cout_stored;
        p.cin_stored = cin_stored;
        size_t bytes;
        if (kind == P_CONV_W) bytes = (size_t)cout_stored * ks * ks * p.cin_stored * dtype_size(dtype);
        else if (kind == P_DW_W) bytes = (size_t)49 * cout * sizeof(float);
        else bytes = (size_t)cout_stored * sizeof(float);
        AP_HIP_CHECK(hipMalloc(&p.d, bytes));
        DevParam& slot = params_[name] = p;
        AP_HIP_CHECK(hipMemset(slot.d, 0, bytes));
        *out = &slot;
        return AP_OK;
    }

    // ap_<who>_set_param: host f32 in torch layout -> the device layout of the parameter's kind
    int set(const char* who, const char* name, const float* host, size_t count) {
        auto it = params_.find(name);
        AP_REQUIRE(it != params_.end(), "%s_set_param: unknown parameter '%s'", who, name);
        DevParam& p = it->second;
        AP_REQUIRE(count == p.torch_count(), "%s_set_param: %s has %zu values, expected %zu", who, name, count, p.torch_count());
        if (p.kind == P_VEC) {
            AP_HIP_CHECK(hipMemcpy(p.d, host, count * sizeof(float), hipMemcpyHostToDevice));
        } else if (p.kind == P_DW_W) {
            // torch [C][1][7][7] -> f32 [49][C]
            std::vector<float> t((size_t)49 * p.cout);
            for (int ch = 0; ch < p.cout; ++ch)
                for (int k = 0; k < 49; ++k) t[(size_t)k * p.cout + ch] = host[(size_t)ch * 49 + k];
            AP_HIP_CHECK(hipMemcpy(p.d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
        } else {
            const int rc = upload_conv_weight(who, name, p, host);
            if (rc != AP_OK) return rc;
        }
        p.set = true;
        return AP_OK;
    }

    // ap_<who>_finalize: every parameter has been set
    int check_all_set(const char* who) const {
        for (auto& kv : params_) {
            if (!kv.second.set) {
                set_error("%s_finalize: parameter '%s' was never set", who, kv.first.c_str());
                return AP_ERR_STATE;
            }
        }
        return AP_OK;
    }

  private:
    std::map<std::string, DevParam> params_;

    // torch [cout][cin][ky][kx] -> [cout_stored][ky][kx][cin_stored] (zero channels past cin, zero rows past cout), then to T
    // on the device
    int upload_conv_weight(const char* who, const char* name, DevParam& p, const float* host) {
        const size_t elems = (size_t)p.cout_stored * p.ks * p.ks * p.cin_stored;
        std::vector<float> perm(elems, 0.f);
        for (int o = 0; o < p.cout; ++o)
            for (int ci = 0; ci < p.cin; ++ci)
                for (int ky = 0; ky < p.ks; ++ky)
                    for (int kx = 0; kx < p.ks; ++kx)
                        perm[(((size_t)o * p.ks + ky) * p.ks + kx) * p.cin_stored + ci] =
                            host[(((size_t)o * p.cin + ci) * p.ks + ky) * p.ks + kx];
        float* tmp = nullptr;
        AP_HIP_CHECK(hipMalloc((void**)&tmp, elems * sizeof(float)));
        int rc = AP_OK;
        if (hipMemcpy(tmp, perm.data(), elems * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("%s_set_param: hipMemcpy of %s failed", who, name);
            rc = AP_ERR_HIP;
        }
        if (rc == AP_OK) rc = launch_convert(dtype, tmp, p.d, elems, nullptr);
        if (rc == AP_OK && hipDeviceSynchronize() != hipSuccess) {
            set_error("%s_set_param: conversion of %s failed", who, name);
            rc = AP_ERR_HIP;
        }
        (void)hipFree(tmp);
        return rc;
    }
};

// ---- a convolution / linear layer of an engine, resolved at create: "<name>.weight" and "<name>.bias" (null: bias-free)
struct Conv {
    DevParam* w = nullptr;      // T [cout_stored][ks][ks][cin_stored]
    DevParam* b = nullptr;      // f32 [cout_stored]
};

inline int add_conv(ParamStore& store, const std::string& name, int cout, int cin, int ks, int cout_stored, int cin_stored,
                    Conv* out) {
    const int rc = store.add_padded(name + ".weight", P_CONV_W, cout, cin, ks, cout_stored, cin_stored, &out->w);
    return rc != AP_OK ? rc : store.add_padded(name + ".bias", P_VEC, cout, 0, 0, cout_stored, 0, &out->b);
}

inline int add_conv(ParamStore& store, const std::string& name, int cout, int cin, int ks, Conv* out) {   // unpadded
    return add_conv(store, name, cout, cin, ks, cout, (int)align_up(cin, 8), out);
}

// ---- the bodies of ap_<who>_set_param / ap_<who>_finalize and the dtype check of ap_<who>_create, for an engine that keeps
// its parameters in `params` (a ParamStore) and a `finalized` flag
template <class Engine>
int set_param(Engine* m, const char* who, const char* name, const float* host, size_t count) {
    AP_REQUIRE(m && name && host, "%s_set_param: null argument", who);
    const int rc = m->params.set(who, name, host, count);
    if (rc == AP_OK) m->finalized = false;
    return rc;
}

template <class Engine>
int finalize(Engine* m, const char* who) {
    AP_REQUIRE(m, "%s_finalize: null handle", who);
    const int rc = m->params.check_all_set(who);
    if (rc == AP_OK) m->finalized = true;
    return rc;
}

inline int check_compute_dtype(const char* who, int dtype) {
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16 || dtype == AP_F32, "%s_create: compute dtype %d", who, dtype);
    return AP_OK;
}

}  // namespace ap
