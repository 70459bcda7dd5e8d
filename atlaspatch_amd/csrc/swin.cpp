// Swin encoder object behind the C ABI (ap_swin_*): the CHIEF-CTransPath network -- a Swin-Tiny with a convolutional stem.
// Parameter storage in HBM, workspace carving and the launch sequence of one forward pass.  Host C++ only; the kernels live in
// swin.hip (shifted-window attention, patch merging + LayerNorm), convnext.hip (LayerNorm rows) and conv.hip (preprocess,
// implicit-GEMM convolution with the GELU / residual epilogues, average pool).
//
// Forward for n images (T = compute dtype, NHWC everywhere, C_s = embed_dim 2^s, H_0 = S / 4):
//   preprocess  u8 tiles -> centre crop -> normalised T [n, S, S, 8] (channels 3..7 zero)
//   stem        conv 3x3 s2 p1 + ReLU -> [n, S/2, S/2, 32]; conv 3x3 s2 p1 + ReLU -> [n, H_0, H_0, 32]; conv 1x1 -> C_0;
//               LayerNorm.  BatchNorm is folded by the caller; the 12 / 24 output channels are stored padded to 32 with zero
//               weights and zero bias (ParamStore::add_padded; the padded channels stay exactly 0 through the ReLU), so all
//               three run on the implicit GEMM
//   stage s     (s > 0: patch merging = 2x2 gather + LayerNorm(4 C_{s-1}) in one kernel, then the bias-free reduction as a
//               1x1 convolution against a zero bias), then depths[s] blocks, block j with shift 0 (j even, or the map is one
//               window) or 3:
//                 t = LN1(x); qkv = t Wqkv^T + b; a = WA(qkv, shift, bias table of the block); x' = x + a Wproj^T + b
//                 t = LN2(x'); h = GELU(t W1^T + b1); x = x' + h W2^T + b2
//   head        LayerNorm(C_3), global average pool -> f32 [n, C_3]
// Workspace: three buffers of the largest [H, H, C] activation (stream, LayerNorm / attention output, the stream after the
// attention half) and one of the largest [H, H, 4C] hidden tensor, which also holds qkv and the stem's first two tensors.
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include "engine_host.h"

namespace {

constexpr float LN_EPS = 1e-5f;
constexpr int WINDOW = 7, HEAD_DIM = 32, BIAS_TABLE = 169;

using ap::Conv;
using ap::DevParam;
using ap::ParamKind;
using ap::P_CONV_W;
using ap::P_VEC;
using ap::ScopedTimer;

struct Norm {
    DevParam *w = nullptr, *b = nullptr;
};

struct Block {
    Norm ln1, ln2;
    Conv qkv, proj, fc1, fc2;
    DevParam* rel_bias = nullptr;   // f32 [heads][49][49], expanded from the [169, heads] table by ap_swin_set_param
};

struct Stage {
    int c = 0, heads = 0;
    Norm merge_ln;                  // stages 1..3: LayerNorm(4 C_{s-1}) of the patch merging
    Conv reduction;                 // ... and its Linear(4 C_{s-1} -> C_s), no bias
    std::vector<Block> blocks;
};

}  // namespace

struct ap_swin {
    ap_swin_config cfg;
    ap::ParamStore params;
    Conv stem[3];
    Norm stem_ln, final_ln;
    Stage stages[4];
    std::map<std::string, int> bias_tables;     // relative_position_bias_table name -> heads: expanded on upload
    float* zero_bias = nullptr;                 // f32 [C_3] zeros: the reduction layers have no bias
    size_t small_elems = 0;     // elements per image of the largest [H, H, C] activation
    size_t big_elems = 0;       // ... of the largest [H, H, 4C] hidden tensor
    bool finalized = false;
    ap::LaunchProfiler prof;
    ~ap_swin() {
        if (zero_bias) (void)hipFree(zero_bias);
    }
};

namespace {

size_t align256(size_t v) { return ap::align_up(v, 256); }

// a bias-free layer (c.b null) runs against the engine's zero bias
int run_conv(ap_swin* m, const Conv& c, const void* x, int n, int h, int stride, int pad, const void* resid, int act, void* out,
             hipStream_t s) {
    const DevParam& w = *c.w;
    return ap::launch_conv2d_nhwc_ex(m->cfg.compute_dtype, x, n, h, h, w.cin_stored, w.d, c.b ? (const float*)c.b->d : m->zero_bias,
                                     w.cout_stored, w.ks, stride, pad, resid, act, out, s);
}

int run_ln(ap_swin* m, const Norm& ln, const void* x, int rows, int c, void* out, hipStream_t s) {
    return ap::launch_layernorm_rows(m->cfg.compute_dtype, x, rows, c, (const float*)ln.w->d, (const float*)ln.b->d, LN_EPS, out, s);
}

}  // namespace

extern "C" {

size_t ap_sizeof_swin_config(void) { return sizeof(ap_swin_config); }

int ap_swin_config_init(ap_swin_config* cfg, size_t sizeof_caller) {
    return ap::config_init("swin", cfg, sizeof_caller, AP_SWIN_CONFIG_SIZE_V20);
}

int ap_swin_create(const ap_swin_config* cfg, ap_swin** out) {
    AP_REQUIRE(cfg && out, "swin_create: null argument");
    static_assert(sizeof(ap_swin_config) == AP_SWIN_CONFIG_SIZE_V20, "ap_swin_config grew: append only, list the sizes it has had");
    ap_swin_config c;
    int rc = ap::accept_config("swin", cfg, 4096, "", &c);
    if (rc != AP_OK) return rc;
    AP_REQUIRE(c.window == WINDOW, "swin_create: window %d (the kernels are written for 7)", c.window);
    AP_REQUIRE(c.embed_dim >= 32 && c.embed_dim % 32 == 0 && c.embed_dim <= 512, "swin_create: embed_dim %d (a multiple of 32)",
               c.embed_dim);
    for (int s = 0; s < 4; ++s) {
        AP_REQUIRE(c.depths[s] >= 1 && c.depths[s] <= 64, "swin_create: depths[%d] = %d", s, c.depths[s]);
        AP_REQUIRE(c.heads[s] >= 1 && (c.embed_dim << s) == c.heads[s] * HEAD_DIM,
                   "swin_create: stage %d has width %d and %d heads (the head dimension must be 32)", s, c.embed_dim << s, c.heads[s]);
    }
    if ((rc = ap::check_compute_dtype("swin", c.compute_dtype)) != AP_OK) return rc;
    AP_REQUIRE(c.image_size >= 224 && c.image_size <= 896 && c.image_size % 224 == 0,
               "swin_create: image_size %d (a multiple of 224: every stage's map is whole 7x7 windows)", c.image_size);
    ap_swin* m = new ap_swin();
    m->cfg = c;
    m->params.dtype = c.compute_dtype;
    auto add = [&](const std::string& name, ParamKind kind, int cout, int cin, int ks, DevParam** p) {
        if (rc == AP_OK) rc = m->params.add(name, kind, cout, cin, ks, p);
    };
    auto add_norm = [&](const std::string& pre, int width, Norm* ln) {
        add(pre + ".weight", P_VEC, width, 0, 0, &ln->w);
        add(pre + ".bias", P_VEC, width, 0, 0, &ln->b);
    };
    auto add_linear = [&](const std::string& pre, int cout, int cin, Conv* l) {
        if (rc == AP_OK) rc = ap::add_conv(m->params, pre, cout, cin, 1, l);
    };
    // the stem: Cout stored as the next multiple of 32, Cin as the producing map's stored channels (the image: 8)
    auto add_stem = [&](const std::string& pre, int cout, int cin, int ks, int cin_p, Conv* l) {
        if (rc == AP_OK) rc = ap::add_conv(m->params, pre, cout, cin, ks, (int)ap::align_up((size_t)cout, 32), cin_p, l);
    };
    const int S = c.image_size, E = c.embed_dim;
    const int c1 = E / 8, c2 = E / 4, c1p = (int)ap::align_up((size_t)c1, 32), c2p = (int)ap::align_up((size_t)c2, 32);
    add_stem("patch_embed.proj.0", c1, 3, 3, 8, &m->stem[0]);
    add_stem("patch_embed.proj.3", c2, c1, 3, c1p, &m->stem[1]);
    add_stem("patch_embed.proj.6", E, c2, 1, c2p, &m->stem[2]);
    add_norm("patch_embed.norm", E, &m->stem_ln);
    size_t small = 0, big = (size_t)S * S * 8 + (size_t)(S / 2) * (S / 2) * c1p + 128;   // + the 256-byte alignment slack
    small = (size_t)(S / 4) * (S / 4) * c2p;
    int hw = S / 4;
    for (int s = 0; s < 4; ++s) {
        Stage& st = m->stages[s];
        const int C = E << s;
        st.c = C;
        st.heads = c.heads[s];
        const std::string layer = "layers." + std::to_string(s) + ".";
        if (s > 0) {
            add_norm(layer + "downsample.norm", 2 * C, &st.merge_ln);
            add(layer + "downsample.reduction.weight", P_CONV_W, C, 2 * C, 1, &st.reduction.w);
            hw /= 2;
        }
        small = std::max(small, (size_t)hw * hw * C);
        big = std::max(big, (size_t)hw * hw * 4 * C);
        st.blocks.resize(c.depths[s]);
        for (int j = 0; j < c.depths[s]; ++j) {
            Block& b = st.blocks[j];
            const std::string pre = layer + "blocks." + std::to_string(j) + ".";
            add_norm(pre + "norm1", C, &b.ln1);
            add_linear(pre + "attn.qkv", 3 * C, C, &b.qkv);
            add(pre + "attn.relative_position_bias_table", P_VEC, st.heads * 49 * 49, 0, 0, &b.rel_bias);
            m->bias_tables[pre + "attn.relative_position_bias_table"] = st.heads;
            add_linear(pre + "attn.proj", C, C, &b.proj);
            add_norm(pre + "norm2", C, &b.ln2);
            add_linear(pre + "mlp.fc1", 4 * C, C, &b.fc1);
            add_linear(pre + "mlp.fc2", C, 4 * C, &b.fc2);
        }
    }
    add_norm("norm", E << 3, &m->final_ln);
    m->small_elems = small;
    m->big_elems = big;
    if (rc == AP_OK) {
        const size_t bytes = (size_t)(E << 3) * sizeof(float);
        if (hipMalloc((void**)&m->zero_bias, bytes) != hipSuccess || hipMemset(m->zero_bias, 0, bytes) != hipSuccess) {
            ap::set_error("swin_create: allocating the zero bias failed");
            rc = AP_ERR_HIP;
        }
    }
    if (rc != AP_OK) { delete m; return rc; }
    *out = m;
    return AP_OK;
}

void ap_swin_destroy(ap_swin* m) { delete m; }

int ap_swin_set_param(ap_swin* m, const char* name, const float* host, size_t count) {
    if (!m || !name || !host || !m->bias_tables.count(name)) return ap::set_param(m, "swin", name, host, count);
    // timm's relative_position_bias_table [169, heads] -> f32 [heads][49][49]: B_h[i, j] = table[(yi - yj + 6) 13 + (xi - xj + 6), h]
    const int heads = m->bias_tables[name];
    AP_REQUIRE(count == (size_t)BIAS_TABLE * heads, "swin_set_param: %s has %zu values, expected %zu", name, count,
               (size_t)BIAS_TABLE * heads);
    std::vector<float> t((size_t)heads * 49 * 49);
    for (int h = 0; h < heads; ++h)
        for (int i = 0; i < 49; ++i)
            for (int j = 0; j < 49; ++j) {
                const int idx = (i / 7 - j / 7 + 6) * 13 + (i % 7 - j % 7 + 6);
                t[((size_t)h * 49 + i) * 49 + j] = host[(size_t)idx * heads + h];
            }
    return ap::set_param(m, "swin", name, t.data(), t.size());
}

int ap_swin_finalize(ap_swin* m) { return ap::finalize(m, "swin"); }

size_t ap_swin_workspace_bytes(const ap_swin* m, int n) {
    if (!m || n <= 0) return 0;
    const size_t ds = ap::dtype_size(m->cfg.compute_dtype);
    return 3 * align256(m->small_elems * (size_t)n * ds) + align256(m->big_elems * (size_t)n * ds);
}

int ap_swin_embed_dim(const ap_swin* m) { return m ? m->cfg.embed_dim << 3 : 0; }

int ap_swin_profile_enable(ap_swin* m, int on) { return ap::profile_enable(m ? &m->prof : nullptr, "swin", on); }

int ap_swin_profile_read(ap_swin* m, double* ms_by_kind, long long* launches_by_kind, int kinds) {
    return ap::profile_read(m ? &m->prof : nullptr, "swin", AP_SWIN_PROF_KINDS, ms_by_kind, launches_by_kind, kinds);
}

int ap_swin_forward_u8(ap_swin* m, const uint8_t* patches, int n, int h, int w, const float mean[3], const float stdv[3], float* out,
                       void* workspace, size_t workspace_bytes, ap_stream_t stream) {
    int rc = ap::check_forward_args("swin", m, n, patches && out && mean && stdv, workspace, workspace_bytes, ap_swin_workspace_bytes);
    if (rc != AP_OK || n == 0) return rc;
    const int S = m->cfg.image_size;
    AP_REQUIRE(h >= S && w >= S, "swin_forward_u8: %dx%d tiles smaller than the %d model input", h, w, S);
    hipStream_t s = (hipStream_t)stream;
    const int dt = m->cfg.compute_dtype;
    const size_t ds = ap::dtype_size(dt);
    const size_t small = align256(m->small_elems * (size_t)n * ds);
    char* xb = (char*)workspace;                    // the residual stream
    char* tb = xb + small;                          // LayerNorm output, then the attention output
    char* ab = tb + small;                          // the stream after the attention half
    char* hb = ab + small;                          // qkv, then the 4C hidden tensor (and the stem's first two tensors)

    int hw = S / 4;
    {
        ScopedTimer t(m->prof, AP_SWIN_PROF_STEM, s);
        char* s1 = hb + align256((size_t)n * S * S * 8 * ds);
        rc = ap::launch_preproc_nhwc8(patches, n, h, w, ap::center_crop_offset(h, S), ap::center_crop_offset(w, S), S, mean, stdv,
                                      hb, dt, s);
        if (rc == AP_OK) rc = run_conv(m, m->stem[0], hb, n, S, 2, 1, nullptr, 1, s1, s);
        if (rc == AP_OK) rc = run_conv(m, m->stem[1], s1, n, S / 2, 2, 1, nullptr, 1, tb, s);
        if (rc == AP_OK) rc = run_conv(m, m->stem[2], tb, n, hw, 1, 0, nullptr, 0, ab, s);
        if (rc == AP_OK) rc = run_ln(m, m->stem_ln, ab, n * hw * hw, m->cfg.embed_dim, xb, s);
    }
    if (rc != AP_OK) return rc;
    for (int si = 0; si < 4; ++si) {
        const Stage& st = m->stages[si];
        const int C = st.c;
        if (si > 0) {
            ScopedTimer t(m->prof, AP_SWIN_PROF_MERGE, s);
            rc = ap::launch_patch_merge_ln(dt, xb, n, hw, hw, C / 2, (const float*)st.merge_ln.w->d, (const float*)st.merge_ln.b->d,
                                           LN_EPS, tb, s);
            hw /= 2;
            if (rc == AP_OK) rc = run_conv(m, st.reduction, tb, n, hw, 1, 0, nullptr, 0, xb, s);
            if (rc != AP_OK) return rc;
        }
        const int rows = n * hw * hw;
        for (size_t j = 0; j < st.blocks.size(); ++j) {
            const Block& b = st.blocks[j];
            const int shift = (j % 2 == 1 && hw > WINDOW) ? WINDOW / 2 : 0;
            {
                ScopedTimer t(m->prof, AP_SWIN_PROF_LN, s);
                rc = run_ln(m, b.ln1, xb, rows, C, tb, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m->prof, AP_SWIN_PROF_QKV, s);
                rc = run_conv(m, b.qkv, tb, n, hw, 1, 0, nullptr, 0, hb, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m->prof, AP_SWIN_PROF_WINDOW_ATTN, s);
                rc = ap::launch_swin_window_attention(dt, hb, n, hw, hw, st.heads, shift, (const float*)b.rel_bias->d, tb, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m->prof, AP_SWIN_PROF_PROJ, s);
                rc = run_conv(m, b.proj, tb, n, hw, 1, 0, xb, 0, ab, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m->prof, AP_SWIN_PROF_LN, s);
                rc = run_ln(m, b.ln2, ab, rows, C, tb, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m->prof, AP_SWIN_PROF_FC1, s);
                rc = run_conv(m, b.fc1, tb, n, hw, 1, 0, nullptr, 2, hb, s);
            }
            if (rc != AP_OK) return rc;
            {
                ScopedTimer t(m->prof, AP_SWIN_PROF_FC2, s);
                rc = run_conv(m, b.fc2, hb, n, hw, 1, 0, ab, 0, xb, s);
            }
            if (rc != AP_OK) return rc;
        }
    }
    {
        ScopedTimer t(m->prof, AP_SWIN_PROF_LN, s);
        rc = run_ln(m, m->final_ln, xb, n * hw * hw, m->cfg.embed_dim << 3, tb, s);
    }
    if (rc != AP_OK) return rc;
    ScopedTimer t(m->prof, AP_SWIN_PROF_POOL, s);
    return ap::launch_avgpool_nhwc(dt, tb, n, hw * hw, m->cfg.embed_dim << 3, out, s);
}

}  // extern "C"
