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
#include <string>
#include <vector>
#include "engine_host.h"

namespace {

constexpr float LN_EPS = 1e-6f;

using ap::Conv;
using ap::DevParam;
using ap::ParamKind;
using ap::P_DW_W;
using ap::P_VEC;
using ap::ScopedTimer;

struct Block {
    DevParam *dw_w, *dw_b, *ln_w, *ln_b;
    Conv fc1, fc2;
};

struct Stage {
    int c = 0;
    DevParam *ds_ln_w = nullptr, *ds_ln_b = nullptr;   // stages 1..3: the downsampling LayerNorm
    Conv ds;                                             // ... and its 2x2 stride-2 convolution
    std::vector<Block> blocks;
};

}  // namespace

struct ap_convnext {
    ap_convnext_config cfg;
    ap::ParamStore params;
    Conv stem;
    DevParam *stem_ln_w = nullptr, *stem_ln_b = nullptr;
    Stage stages[4];
    size_t small_elems = 0;     // elements per image of the largest [H, H, C] activation
    size_t big_elems = 0;       // ... of the largest [H, H, 4C] hidden tensor (and the stem input)
    bool finalized = false;
    ap::LaunchProfiler prof;
};

namespace {

size_t align256(size_t v) { return ap::align_up(v, 256); }

int run_conv(ap_convnext* m, const Conv& c, const void* x, int n, int h, int stride, const void* resid, int act, void* out,
             hipStream_t s) {
    const DevParam& w = *c.w;
    return ap::launch_conv2d_nhwc_ex(m->cfg.compute_dtype, x, n, h, h, w.cin_stored, w.d, (const float*)c.b->d, w.cout, w.ks,
                                     stride, 0, resid, act, out, s);
}

}  // namespace

extern "C" {

size_t ap_sizeof_convnext_config(void) { return sizeof(ap_convnext_config); }

int ap_convnext_config_init(ap_convnext_config* cfg, size_t sizeof_caller) {
    return ap::config_init("convnext", cfg, sizeof_caller, AP_CONVNEXT_CONFIG_SIZE_V20);
}

int ap_convnext_create(const ap_convnext_config* cfg, ap_convnext** out) {
    AP_REQUIRE(cfg && out, "convnext_create: null argument");
    static_assert(sizeof(ap_convnext_config) == AP_CONVNEXT_CONFIG_SIZE_V20,
                  "ap_convnext_config grew: append only, list the sizes it has had");
    ap_convnext_config c;
    int rc = ap::accept_config("convnext", cfg, 4096, "", &c);
    if (rc != AP_OK) return rc;
    for (int s = 0; s < 4; ++s) {
        AP_REQUIRE(c.depths[s] >= 1 && c.depths[s] <= 64, "convnext_create: depths[%d] = %d", s, c.depths[s]);
        AP_REQUIRE(c.widths[s] >= 32 && c.widths[s] % 32 == 0 && c.widths[s] <= 4096,
                   "convnext_create: widths[%d] = %d (a multiple of 32)", s, c.widths[s]);
    }
    if ((rc = ap::check_compute_dtype("convnext", c.compute_dtype)) != AP_OK) return rc;
    AP_REQUIRE(c.image_size >= 32 && c.image_size <= 1024 && c.image_size % 32 == 0,
               "convnext_create: image_size %d (a multiple of 32)", c.image_size);
    ap_convnext* m = new ap_convnext();
    m->cfg = c;
    m->params.dtype = c.compute_dtype;
    auto add = [&](const std::string& name, ParamKind kind, int cout, int cin, int ks, DevParam** p) {
        if (rc == AP_OK) rc = m->params.add(name, kind, cout, cin, ks, p);
    };
    auto add_conv = [&](const std::string& name, int cout, int cin, int ks, Conv* l) {
        if (rc == AP_OK) rc = ap::add_conv(m->params, name, cout, cin, ks, l);
    };
    const int S = c.image_size;
    add_conv("features.0.0", c.widths[0], 3, 4, &m->stem);
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
            add_conv(d + "1", C, c.widths[s - 1], 2, &st.ds);
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
            add_conv(pre + "3", 4 * C, C, 1, &b.fc1);
            add_conv(pre + "5", C, 4 * C, 1, &b.fc2);
        }
    }
    m->small_elems = small;
    m->big_elems = big;
    if (rc != AP_OK) { delete m; return rc; }
    *out = m;
    return AP_OK;
}

void ap_convnext_destroy(ap_convnext* m) { delete m; }

int ap_convnext_set_param(ap_convnext* m, const char* name, const float* host, size_t count) {
    return ap::set_param(m, "convnext", name, host, count);
}

int ap_convnext_finalize(ap_convnext* m) { return ap::finalize(m, "convnext"); }

size_t ap_convnext_workspace_bytes(const ap_convnext* m, int n) {
    if (!m || n <= 0) return 0;
    const size_t ds = ap::dtype_size(m->cfg.compute_dtype);
    return 2 * align256(m->small_elems * (size_t)n * ds) + align256(m->big_elems * (size_t)n * ds);
}

int ap_convnext_embed_dim(const ap_convnext* m) { return m ? m->cfg.widths[3] : 0; }

int ap_convnext_profile_enable(ap_convnext* m, int on) { return ap::profile_enable(m ? &m->prof : nullptr, "convnext", on); }

int ap_convnext_profile_read(ap_convnext* m, double* ms_by_kind, long long* launches_by_kind, int kinds) {
    return ap::profile_read(m ? &m->prof : nullptr, "convnext", AP_CONVNEXT_PROF_KINDS, ms_by_kind, launches_by_kind, kinds);
}

int ap_convnext_forward_u8(ap_convnext* m, const uint8_t* patches, int n, int h, int w, const float mean[3], const float stdv[3],
                           float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream) {
    int rc = ap::check_forward_args("convnext", m, n, patches && out && mean && stdv, workspace, workspace_bytes,
                                    ap_convnext_workspace_bytes);
    if (rc != AP_OK || n == 0) return rc;
    const int S = m->cfg.image_size;
    AP_REQUIRE(h >= S && w >= S, "convnext_forward_u8: %dx%d tiles smaller than the %d model input", h, w, S);
    hipStream_t s = (hipStream_t)stream;
    const int dt = m->cfg.compute_dtype;
    const size_t ds = ap::dtype_size(dt);
    const size_t small = align256(m->small_elems * (size_t)n * ds);
    char* xb = (char*)workspace;                    // the residual stream
    char* tb = xb + small;                          // LN output, then the block's new stream
    char* hb = tb + small;                          // the 4C hidden tensor (and the stem input)

    int hw = S / 4;
    {
        ScopedTimer t(m->prof, AP_CONVNEXT_PROF_STEM, s);
        rc = ap::launch_preproc_nhwc8(patches, n, h, w, ap::center_crop_offset(h, S), ap::center_crop_offset(w, S), S, mean, stdv,
                                      hb, dt, s);
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
            ScopedTimer t(m->prof, AP_CONVNEXT_PROF_DOWNSAMPLE, s);
            const int cprev = m->stages[si - 1].c;
            rc = ap::launch_layernorm_rows(dt, xb, n * hw * hw, cprev, (const float*)st.ds_ln_w->d, (const float*)st.ds_ln_b->d,
                                           LN_EPS, tb, s);
            if (rc == AP_OK) rc = run_conv(m, st.ds, tb, n, hw, 2, nullptr, 0, xb, s);
            if (rc != AP_OK) return rc;
            hw /= 2;
        }
        for (const Block& b : st.blocks) {
            {
                ScopedTimer t(m->prof, AP_CONVNEXT_PROF_DWCONV_LN, s);
                rc = ap::launch_dwconv7_ln_nhwc(dt, xb, n, hw, hw, C, (const float*)b.dw_w->d, (const float*)b.dw_b->d,
                                                (const float*)b.ln_w->d, (const float*)b.ln_b->d, LN_EPS, tb, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m->prof, AP_CONVNEXT_PROF_FC1, s);
                rc = run_conv(m, b.fc1, tb, n, hw, 1, nullptr, 2, hb, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m->prof, AP_CONVNEXT_PROF_FC2, s);
                rc = run_conv(m, b.fc2, hb, n, hw, 1, xb, 0, tb, s);
            }
            if (rc != AP_OK) return rc;
            std::swap(xb, tb);
        }
    }
    ScopedTimer t(m->prof, AP_CONVNEXT_PROF_POOL, s);
    return ap::launch_avgpool_nhwc(dt, xb, n, hw * hw, m->cfg.widths[3], out, s);
}

}  // extern "C"
