// ConvNeXt encoder object behind the C ABI (ap_convnext_*): parameter storage in HBM, workspace carving and the launch
// sequence of one forward pass.  Host C++ only; the kernels live in convnext.hip (depthwise 7x7 + LayerNorm, LayerNorm rows)
// and conv.hip (preprocess, implicit-GEMM convolution with the 32-wide N tail and the GELU epilogue, average pool).
//
// Forward for n images (T = compute dtype, NHWC everywhere, C_s = widths[s], H_0 = S / 4):
//   preprocess  u8 tiles -> centre crop -> normalised T [n, S, S, 8] (channels 3..7 zero)
//   stem        conv 4x4 s4 (+ bias) -> [n, H_0, H_0, C_0]; LayerNorm over the channels
//   stage s     (s > 0: LayerNorm -> conv 2x2 s2 (+ bias), C_{s-1} -> C_s), then depths[s] blocks:
//                 t = LN(dwconv7x7(x))        dwconv7_ln, one kernel
//                 h = GELU(t W1^T + b1)       implicit GEMM, ks = 1, GELU epilogue        [n, H, H, 4C]
//                 x = x + h W2'^T + b2'       implicit GEMM, ks = 1, residual epilogue    (layer_scale folded into W2', b2')
//   head        global average pool -> f32 [n, C_3]   (no final LayerNorm: the reference replaces the whole classifier)
// Workspace: three buffers -- two of the largest [H, H, C] activation (the residual stream and the block's LN output / next
// stream, swapped every block) and one of the largest [H, H, 4C] hidden tensor, which also holds the preprocessed stem input.
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "ap_common.h"

namespace {

constexpr float LN_EPS = 1e-6f;

enum ParamKind { P_CONV_W, P_DW_W, P_VEC };

struct Param {
    ParamKind kind = P_VEC;
    int cout = 0, cin = 0, cin_stored = 0, ks = 0;   // P_CONV_W: torch [cout, cin, ks, ks]; P_DW_W: [cout, 1, 7, 7]; P_VEC: [cout]
    void* d = nullptr;          // P_CONV_W: T [cout][ks][ks][cin_stored]; P_DW_W: f32 [49][cout]; P_VEC: f32 [cout]
    bool set = false;
    size_t torch_count() const { return kind == P_VEC ? (size_t)cout : (size_t)cout * cin * ks * ks; }
};

struct Conv {                   // a convolution / linear layer: weight and bias
    Param* w = nullptr;
    Param* b = nullptr;
};

struct Block {
    Param *dw_w, *dw_b, *ln_w, *ln_b;
    Conv fc1, fc2;
};

struct Stage {
    int c = 0;
    Param *ds_ln_w = nullptr, *ds_ln_b = nullptr;   // stages 1..3: the downsampling LayerNorm
    Conv ds;                                         // ... and its 2x2 stride-2 convolution
    std::vector<Block> blocks;
};

}  // namespace

struct ap_convnext {
    ap_convnext_config cfg;
    std::map<std::string, Param> params;
    Conv stem;
    Param *stem_ln_w = nullptr, *stem_ln_b = nullptr;
    Stage stages[4];
    size_t small_elems = 0;     // elements per image of the largest [H, H, C] activation
    size_t big_elems = 0;       // ... of the largest [H, H, 4C] hidden tensor (and the stem input)
    bool finalized = false;
    bool profile = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_used;
    size_t ev_next = 0;
};

namespace {

hipEvent_t next_event(ap_convnext* m) {
    if (m->ev_next == m->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        m->ev_pool.push_back(e);
    }
    return m->ev_pool[m->ev_next++];
}
struct ScopedTimer {      // records start/stop events around one launch group when profiling is on
    ap_convnext* m; int kind; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(ap_convnext* m_, int kind_, hipStream_t s_) : m(m_), kind(kind_), s(s_) {
        if (m->profile) { a = next_event(m); b = next_event(m); if (a) (void)hipEventRecord(a, s); }
    }
    ~ScopedTimer() {
        if (m->profile && a && b) { (void)hipEventRecord(b, s); m->ev_used.push_back({kind, {a, b}}); }
    }
};

int add_param(ap_convnext* m, const std::string& name, ParamKind kind, int cout, int cin, int ks, Param** out) {
    Param p;
    p.kind = kind; p.cout = cout; p.cin = cin; p.ks = ks;
    p.cin_stored = kind == P_CONV_W ? (int)ap::align_up(cin, 8) : cin;
    size_t bytes;
    if (kind == P_CONV_W) bytes = (size_t)cout * ks * ks * p.cin_stored * ap::dtype_size(m->cfg.compute_dtype);
    else if (kind == P_DW_W) bytes = (size_t)49 * cout * sizeof(float);
    else bytes = (size_t)cout * sizeof(float);
    AP_HIP_CHECK(hipMalloc(&p.d, bytes));
    AP_HIP_CHECK(hipMemset(p.d, 0, bytes));
    m->params[name] = p;
    *out = &m->params[name];        // std::map nodes are stable
    return AP_OK;
}

void free_params(ap_convnext* m) {
    for (auto& kv : m->params)
        if (kv.second.d) (void)hipFree(kv.second.d);
    m->params.clear();
}

size_t align256(size_t v) { return ap::align_up(v, 256); }

int run_conv(ap_convnext* m, const Conv& c, const void* x, int n, int h, int stride, const void* resid, int act, void* out,
             hipStream_t s) {
    const Param& w = *c.w;
    return ap::launch_conv2d_nhwc_ex(m->cfg.compute_dtype, x, n, h, h, w.cin_stored, w.d, (const float*)c.b->d, w.cout, w.ks,
                                     stride, 0, resid, act, out, s);
}

}  // namespace

extern "C" {

size_t ap_sizeof_convnext_config(void) { return sizeof(ap_convnext_config); }

int ap_convnext_config_init(ap_convnext_config* cfg, size_t sizeof_caller) {
    AP_REQUIRE(cfg, "convnext_config_init: null argument");
    AP_REQUIRE(sizeof_caller >= AP_CONVNEXT_CONFIG_SIZE_V20 && sizeof_caller % 4 == 0 && sizeof_caller <= 4096,
               "convnext_config_init: %zu is not the size of an ap_convnext_config (%u bytes, this library: %zu)", sizeof_caller,
               AP_CONVNEXT_CONFIG_SIZE_V20, sizeof(ap_convnext_config));
    memset(cfg, 0, sizeof_caller);
    cfg->struct_size = (uint32_t)sizeof_caller;
    return AP_OK;
}

int ap_convnext_create(const ap_convnext_config* cfg, ap_convnext** out) {
    AP_REQUIRE(cfg && out, "convnext_create: null argument");
    static_assert(sizeof(ap_convnext_config) == AP_CONVNEXT_CONFIG_SIZE_V20,
                  "ap_convnext_config grew: append only, list the sizes it has had");
    const size_t given = cfg->struct_size;
    if (given > sizeof(ap_convnext_config) && given % 4 == 0 && given <= 4096) {
        ap::set_error("convnext_create: cfg->struct_size = %zu is larger than this library's ap_convnext_config (%zu bytes): the "
                      "binding was generated from a newer include/atlaspatch_hip.h than the library was built from", given,
                      sizeof(ap_convnext_config));
        return AP_ERR_UNSUPPORTED;
    }
    AP_REQUIRE(given == AP_CONVNEXT_CONFIG_SIZE_V20,
               "convnext_create: cfg->struct_size = %zu is not a size ap_convnext_config has had (%u bytes): fill the structure "
               "with ap_convnext_config_init(&cfg, sizeof cfg)", given, AP_CONVNEXT_CONFIG_SIZE_V20);
    ap_convnext_config c;
    memcpy(&c, cfg, sizeof(c));
    for (int s = 0; s < 4; ++s) {
        AP_REQUIRE(c.depths[s] >= 1 && c.depths[s] <= 64, "convnext_create: depths[%d] = %d", s, c.depths[s]);
        AP_REQUIRE(c.widths[s] >= 32 && c.widths[s] % 32 == 0 && c.widths[s] <= 4096,
                   "convnext_create: widths[%d] = %d (a multiple of 32)", s, c.widths[s]);
    }
    AP_REQUIRE(c.compute_dtype == AP_F16 || c.compute_dtype == AP_BF16 || c.compute_dtype == AP_F32,
               "convnext_create: compute dtype %d", c.compute_dtype);
    AP_REQUIRE(c.image_size >= 32 && c.image_size <= 1024 && c.image_size % 32 == 0,
               "convnext_create: image_size %d (a multiple of 32)", c.image_size);
    ap_convnext* m = new ap_convnext();
    m->cfg = c;
    int rc = AP_OK;
    auto add = [&](const std::string& name, ParamKind kind, int cout, int cin, int ks, Param** p) {
        if (rc == AP_OK) rc = add_param(m, name, kind, cout, cin, ks, p);
    };
    const int S = c.image_size;
    add("features.0.0.weight", P_CONV_W, c.widths[0], 3, 4, &m->stem.w);
    add("features.0.0.bias", P_VEC, c.widths[0], 0, 0, &m->stem.b);
    add("features.0.1.weight", P_VEC, c.widths[0], 0, 0, &m->stem_ln_w);
    add("features.0.1.bias", P_VEC, c.widths[0], 0, 0, &m->stem_ln_b);
    size_t small = 0, big = (size_t)S * S * 8;
    int hw = S / 4;
    for (int s = 0; s < 4; ++s) {
        Stage& st = m->stages[s];
        const int C = c.widths[s];
        st.c = C;
        if (s > 0) {
            const std::string d = "features." + std::to_string(2 * s) + ".";
            add(d + "0.weight", P_VEC, c.widths[s - 1], 0, 0, &st.ds_ln_w);
            add(d + "0.bias", P_VEC, c.widths[s - 1], 0, 0, &st.ds_ln_b);
            add(d + "1.weight", P_CONV_W, C, c.widths[s - 1], 2, &st.ds.w);
            add(d + "1.bias", P_VEC, C, 0, 0, &st.ds.b);
            hw /= 2;
        }
        small = std::max(small, (size_t)hw * hw * C);
        big = std::max(big, (size_t)hw * hw * 4 * C);
        st.blocks.resize(c.depths[s]);
        for (int j = 0; j < c.depths[s]; ++j) {
            Block& b = st.blocks[j];
            const std::string pre = "features." + std::to_string(2 * s + 1) + "." + std::to_string(j) + ".block.";
            add(pre + "0.weight", P_DW_W, C, 1, 7, &b.dw_w);
            add(pre + "0.bias", P_VEC, C, 0, 0, &b.dw_b);
            add(pre + "2.weight", P_VEC, C, 0, 0, &b.ln_w);
            add(pre + "2.bias", P_VEC, C, 0, 0, &b.ln_b);
            add(pre + "3.weight", P_CONV_W, 4 * C, C, 1, &b.fc1.w);
            add(pre + "3.bias", P_VEC, 4 * C, 0, 0, &b.fc1.b);
            add(pre + "5.weight", P_CONV_W, C, 4 * C, 1, &b.fc2.w);
            add(pre + "5.bias", P_VEC, C, 0, 0, &b.fc2.b);
        }
    }
    m->small_elems = small;
    m->big_elems = big;
    if (rc != AP_OK) { ap_convnext_destroy(m); return rc; }
    *out = m;
    return AP_OK;
}

void ap_convnext_destroy(ap_convnext* m) {
    if (!m) return;
    free_params(m);
    for (hipEvent_t e : m->ev_pool) (void)hipEventDestroy(e);
    delete m;
}

int ap_convnext_set_param(ap_convnext* m, const char* name, const float* host, size_t count) {
    AP_REQUIRE(m && name && host, "convnext_set_param: null argument");
    auto it = m->params.find(name);
    AP_REQUIRE(it != m->params.end(), "convnext_set_param: unknown parameter '%s'", name);
    Param& p = it->second;
    AP_REQUIRE(count == p.torch_count(), "convnext_set_param: %s has %zu values, expected %zu", name, count, p.torch_count());
    if (p.kind == P_VEC) {
        AP_HIP_CHECK(hipMemcpy(p.d, host, count * sizeof(float), hipMemcpyHostToDevice));
    } else if (p.kind == P_DW_W) {
        // torch [C][1][7][7] -> f32 [49][C]
        std::vector<float> t((size_t)49 * p.cout);
        for (int ch = 0; ch < p.cout; ++ch)
            for (int k = 0; k < 49; ++k) t[(size_t)k * p.cout + ch] = host[(size_t)ch * 49 + k];
        AP_HIP_CHECK(hipMemcpy(p.d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    } else {
        // torch [cout][cin][ky][kx] -> [cout][ky][kx][cin_stored] (zero channels past cin), then to T on the device
        const size_t elems = (size_t)p.cout * p.ks * p.ks * p.cin_stored;
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
            ap::set_error("convnext_set_param: hipMemcpy of %s failed", name);
            rc = AP_ERR_HIP;
        }
        if (rc == AP_OK) rc = ap::launch_convert(m->cfg.compute_dtype, tmp, p.d, elems, nullptr);
        if (rc == AP_OK && hipDeviceSynchronize() != hipSuccess) {
            ap::set_error("convnext_set_param: conversion of %s failed", name);
            rc = AP_ERR_HIP;
        }
        (void)hipFree(tmp);
        if (rc != AP_OK) return rc;
    }
    p.set = true;
    m->finalized = false;
    return AP_OK;
}

int ap_convnext_finalize(ap_convnext* m) {
    AP_REQUIRE(m, "convnext_finalize: null handle");
    for (auto& kv : m->params) {
        if (!kv.second.set) {
            ap::set_error("convnext_finalize: parameter '%s' was never set", kv.first.c_str());
            return AP_ERR_STATE;
        }
    }
    m->finalized = true;
    return AP_OK;
}

size_t ap_convnext_workspace_bytes(const ap_convnext* m, int n) {
    if (!m || n <= 0) return 0;
    const size_t ds = ap::dtype_size(m->cfg.compute_dtype);
    return 2 * align256(m->small_elems * (size_t)n * ds) + align256(m->big_elems * (size_t)n * ds);
}

int ap_convnext_embed_dim(const ap_convnext* m) { return m ? m->cfg.widths[3] : 0; }

int ap_convnext_profile_enable(ap_convnext* m, int on) {
    AP_REQUIRE(m, "convnext_profile_enable: null handle");
    m->profile = on != 0;
    m->ev_used.clear();
    m->ev_next = 0;
    return AP_OK;
}

int ap_convnext_profile_read(ap_convnext* m, double* ms_by_kind, long long* launches_by_kind, int kinds) {
    AP_REQUIRE(m && ms_by_kind && launches_by_kind && kinds >= AP_CONVNEXT_PROF_KINDS, "convnext_profile_read: bad arguments");
    for (int k = 0; k < kinds; ++k) { ms_by_kind[k] = 0.0; launches_by_kind[k] = 0; }
    for (auto& u : m->ev_used) {
        AP_HIP_CHECK(hipEventSynchronize(u.second.second));
        float ms = 0.f;
        AP_HIP_CHECK(hipEventElapsedTime(&ms, u.second.first, u.second.second));
        ms_by_kind[u.first] += ms;
        launches_by_kind[u.first] += 1;
    }
    m->ev_used.clear();
    m->ev_next = 0;
    return AP_OK;
}

int ap_convnext_forward_u8(ap_convnext* m, const uint8_t* patches, int n, int h, int w, const float mean[3], const float stdv[3],
                           float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream) {
    AP_REQUIRE(m != nullptr, "convnext: null handle");
    if (!m->finalized) { ap::set_error("convnext: ap_convnext_finalize has not been called"); return AP_ERR_STATE; }
    AP_REQUIRE(n >= 0, "convnext: negative batch");
    if (n == 0) return AP_OK;
    AP_REQUIRE(patches && out && workspace && mean && stdv, "convnext: null buffer");
    AP_REQUIRE(((uintptr_t)workspace & 255) == 0, "convnext: workspace must be 256-byte aligned");
    if (workspace_bytes < ap_convnext_workspace_bytes(m, n)) {
        ap::set_error("convnext: workspace %zu bytes < required %zu", workspace_bytes, ap_convnext_workspace_bytes(m, n));
        return AP_ERR_WORKSPACE;
    }
    const int S = m->cfg.image_size;
    AP_REQUIRE(h >= S && w >= S, "convnext_forward_u8: %dx%d tiles smaller than the %d model input", h, w, S);
    // torchvision CenterCrop: top = int(round((h - S) / 2.0)) (banker's rounding), as ap_vit_forward_u8
    auto crop_off = [](int full, int size) { int d = full - size; return (d / 2) + ((d & 1) && ((d / 2) & 1) ? 1 : 0); };
    hipStream_t s = (hipStream_t)stream;
    const int dt = m->cfg.compute_dtype;
    const size_t ds = ap::dtype_size(dt);
    const size_t small = align256(m->small_elems * (size_t)n * ds);
    char* xb = (char*)workspace;                    // the residual stream
    char* tb = xb + small;                          // LN output, then the block's new stream
    char* hb = tb + small;                          // the 4C hidden tensor (and the stem input)

    int rc;
    int hw = S / 4;
    {
        ScopedTimer t(m, AP_CONVNEXT_PROF_STEM, s);
        rc = ap::launch_preproc_nhwc8(patches, n, h, w, crop_off(h, S), crop_off(w, S), S, mean, stdv, hb, dt, s);
        if (rc == AP_OK) rc = run_conv(m, m->stem, hb, n, S, 4, nullptr, 0, tb, s);
        if (rc == AP_OK)
            rc = ap::launch_layernorm_rows(dt, tb, n * hw * hw, m->cfg.widths[0], (const float*)m->stem_ln_w->d,
                                           (const float*)m->stem_ln_b->d, LN_EPS, xb, s);
    }
    if (rc != AP_OK) return rc;
    for (int si = 0; si < 4; ++si) {
        const Stage& st = m->stages[si];
        const int C = st.c;
        if (si > 0) {
            ScopedTimer t(m, AP_CONVNEXT_PROF_DOWNSAMPLE, s);
            const int cprev = m->stages[si - 1].c;
            rc = ap::launch_layernorm_rows(dt, xb, n * hw * hw, cprev, (const float*)st.ds_ln_w->d, (const float*)st.ds_ln_b->d,
                                           LN_EPS, tb, s);
            if (rc == AP_OK) rc = run_conv(m, st.ds, tb, n, hw, 2, nullptr, 0, xb, s);
            if (rc != AP_OK) return rc;
            hw /= 2;
        }
        for (const Block& b : st.blocks) {
            {
                ScopedTimer t(m, AP_CONVNEXT_PROF_DWCONV_LN, s);
                rc = ap::launch_dwconv7_ln_nhwc(dt, xb, n, hw, hw, C, (const float*)b.dw_w->d, (const float*)b.dw_b->d,
                                                (const float*)b.ln_w->d, (const float*)b.ln_b->d, LN_EPS, tb, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m, AP_CONVNEXT_PROF_FC1, s);
                rc = run_conv(m, b.fc1, tb, n, hw, 1, nullptr, 2, hb, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m, AP_CONVNEXT_PROF_FC2, s);
                rc = run_conv(m, b.fc2, hb, n, hw, 1, xb, 0, tb, s);
            }
            if (rc != AP_OK) return rc;
            std::swap(xb, tb);
        }
    }
    ScopedTimer t(m, AP_CONVNEXT_PROF_POOL, s);
    return ap::launch_avgpool_nhwc(dt, xb, n, hw * hw, m->cfg.widths[3], out, s);
}

}  // extern "C"
