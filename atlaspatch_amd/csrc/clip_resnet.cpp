// OpenAI CLIP "modified ResNet" image tower behind the C ABI (ap_clip_resnet_*): RN50 / RN101 / RN50x4 / RN50x16 / RN50x64.
// Parameter storage in HBM, workspace carving and the launch sequence of one forward pass.  Host C++ only; the kernels live in
// conv.hip (preprocess, implicit-GEMM convolution), clip_resnet.hip (2x2 average pool, token matrix of the head),
// attn_pool.hip (one-query attention) and elementwise.hip (T -> f32).  The block records, the stage walk, the convolution launch
// and the four-buffer workspace are resnet_host.h's, shared with resnet.cpp.
//
// Forward for n images (T = compute dtype, NHWC everywhere, W = width, g = S / 32, C = 32 W):
//   preprocess  u8 tiles -> centre crop -> normalised T [n, S, S, 8] (channels 3..7 zero)
//   stem        conv 3x3 s2 p1 -> W/2, conv 3x3 p1 -> W/2, conv 3x3 p1 -> W (each + folded BN + ReLU), 2x2 average pool
//   stages      bottleneck blocks, planes W 2^s, expansion 4.  Every convolution has stride 1; a block of stride 2 (the first
//               of stages 1..3) average-pools 2x2 behind its 3x3 convolution and in front of its shortcut projection:
//                 t = ReLU(conv1 x); t = ReLU(conv2 t); [t = pool t]; sc = x or downsample([pool] x); x = ReLU(conv3 t + sc)
//   head        tokens [n, g g + 1, C] = (mean token | map) + positional embedding; k | v = one 1x1 convolution to 2C over all
//               tokens; q = the q projection of the n mean-token rows; per head (64 wide) softmax(q k / 8) v; c_proj; T -> f32
// Channel padding: every map is stored with its channel count rounded up to a multiple of 32 (what the implicit GEMM needs of
// Cout; a multiple of 64 takes the ResNet kernel, 32 mod 64 the _ex form).  The weights carry zero rows, a zero bias and zero
// input channels behind the real ones, so a padded channel is exactly 0 through ReLU and the pools and contributes nothing.
//
// Workspace: four buffers of the largest activation each (the stem's input and the head's k | v matrix included), rotated so
// that no launch writes a buffer it reads.  With x the buffer that holds a block's input and f0, f1, f2 the other three:
//   stride 1:  conv1 x -> f0;  conv2 f0 -> f1;  (downsample x -> f2);  conv3 f1 + (f2 | x) -> f0;                  next x = f0
//   stride 2:  conv1 x -> f0;  conv2 f0 -> f1;  pool x -> f0;  downsample f0 -> f2;  pool f1 -> f0;  conv3 f0 + f2 -> f1;  next x = f1
//   stem:      preprocess -> b0;  conv1 b0 -> b1;  conv2 b1 -> b2;  conv3 b2 -> b1;  pool b1 -> b2;               x = b2
//   head:      tokens x -> f0, q rows -> f1;  k | v f0 -> f2;  q f1 -> x;  attention (x, f2) -> f0;  c_proj f0 -> f1;  f1 -> out
#include "resnet_host.h"

using ap::Block;
using ap::ConvOp;
using ap::DevParam;
using ap::ScopedTimer;
using ap::padded32;

namespace {
constexpr int HEAD_DIM = 64;
}

struct ap_clip_resnet {
    ap_clip_resnet_config cfg;
    ap::ParamStore params;
    ConvOp stem[3];
    std::vector<Block> blocks;
    ConvOp q, kv, cproj;
    DevParam* pos = nullptr;    // "attnpool.pos": f32 [g g + 1, C]
    int C = 0, grid = 0;        // the final map: grid x grid pixels of C channels
    size_t max_act = 0;         // elements per image of the largest activation
    bool finalized = false;
    ap::LaunchProfiler prof;
};

namespace {

int run_conv(ap_clip_resnet* m, int kind, const ConvOp& op, const void* x, int n, int hw, const void* resid, int relu, void* out,
             hipStream_t s) {
    return ap::run_conv(m->prof, kind, m->cfg.compute_dtype, op, x, n, hw, hw, resid, relu, out, s);
}

int run_pool(ap_clip_resnet* m, const void* x, int n, int hw, int c, void* out, hipStream_t s) {
    ScopedTimer t(m->prof, AP_CLIP_RESNET_PROF_AVGPOOL, s);
    return ap::launch_avgpool2x2_nhwc(m->cfg.compute_dtype, x, n, hw, hw, c, out, s);
}

inline int conv_kind(const ConvOp& op) { return op.w->ks == 1 ? AP_CLIP_RESNET_PROF_CONV1X1 : AP_CLIP_RESNET_PROF_CONV3X3; }

}  // namespace

extern "C" {

size_t ap_sizeof_clip_resnet_config(void) { return sizeof(ap_clip_resnet_config); }

int ap_clip_resnet_config_init(ap_clip_resnet_config* cfg, size_t sizeof_caller) {
    return ap::config_init("clip_resnet", cfg, sizeof_caller, AP_CLIP_RESNET_CONFIG_SIZE_V20);
}

int ap_clip_resnet_create(const ap_clip_resnet_config* cfg, ap_clip_resnet** out) {
    AP_REQUIRE(cfg && out, "clip_resnet_create: null argument");
    static_assert(sizeof(ap_clip_resnet_config) == AP_CLIP_RESNET_CONFIG_SIZE_V20,
                  "ap_clip_resnet_config grew: append only, list the sizes it has had");
    ap_clip_resnet_config c;
    int rc = ap::accept_config("clip_resnet", cfg, 4096, "", &c);
    if (rc != AP_OK) return rc;
    for (int s = 0; s < 4; ++s)
        AP_REQUIRE(c.depths[s] >= 1 && c.depths[s] <= 64, "clip_resnet_create: depths[%d] = %d (1 .. 64)", s, c.depths[s]);
    AP_REQUIRE(c.width >= 16 && c.width % 16 == 0 && c.width <= 256, "clip_resnet_create: width %d (a multiple of 16, at most 256)",
               c.width);
    AP_REQUIRE(c.image_size >= 64 && c.image_size <= 1024 && c.image_size % 32 == 0,
               "clip_resnet_create: image_size %d (a multiple of 32 in 64 .. 1024: the network reduces it 32-fold)", c.image_size);
    AP_REQUIRE(c.output_dim >= 32 && c.output_dim % 32 == 0 && c.output_dim <= 8192,
               "clip_resnet_create: output_dim %d (a multiple of 32)", c.output_dim);
    if ((rc = ap::check_compute_dtype("clip_resnet", c.compute_dtype)) != AP_OK) return rc;
    ap_clip_resnet* m = new ap_clip_resnet();
    m->cfg = c;
    m->params.dtype = c.compute_dtype;
    // cin_stored: the channel count of the map the convolution reads (its producer's stored Cout; the image: 8)
    auto add = [&](const std::string& name, int cout, int cin, int ks, int cin_stored, ConvOp* op) {
        if (rc == AP_OK) rc = ap::add_conv(m->params, name, cout, cin, ks, padded32(cout), cin_stored, op);
    };
    const int W = c.width, S = c.image_size;
    m->stem[0].stride = 2;
    add("conv1", W / 2, 3, 3, 8, &m->stem[0]);
    add("conv2", W / 2, W / 2, 3, padded32(W / 2), &m->stem[1]);
    add("conv3", W, W / 2, 3, padded32(W / 2), &m->stem[2]);
    ap::Stages st;
    if (rc == AP_OK) rc = ap::add_stages(m->params, {true, W, c.depths, true, false}, W, S / 4, &st);
    m->blocks = std::move(st.blocks);
    m->C = st.channels;
    m->grid = st.hw;
    const int C = m->C, tokens = m->grid * m->grid + 1;
    if (rc == AP_OK) rc = m->params.add("attnpool.pos", ap::P_VEC, tokens * C, 0, 0, &m->pos);
    add("attnpool.q", C, C, 1, C, &m->q);
    add("attnpool.kv", 2 * C, C, 1, C, &m->kv);
    add("attnpool.c", c.output_dim, C, 1, C, &m->cproj);
    // the preprocessed image, the stem's third convolution, the stages and the head's k | v matrix
    m->max_act = std::max({(size_t)S * S * 8, (size_t)(S / 2) * (S / 2) * padded32(W), st.max_act, (size_t)tokens * 2 * C});
    if (rc != AP_OK) { delete m; return rc; }
    *out = m;
    return AP_OK;
}

void ap_clip_resnet_destroy(ap_clip_resnet* m) { delete m; }

int ap_clip_resnet_set_param(ap_clip_resnet* m, const char* name, const float* host, size_t count) {
    if (m && name && std::string(name) == "attnpool.pos") {
        const size_t rows = (size_t)m->grid * m->grid + 1;
        AP_REQUIRE(count == rows * m->C,
                   "clip_resnet_set_param: attnpool.pos has %zu values, expected %zu rows of %d (image_size %d: a %d x %d map and the "
                   "mean token; the positional embedding is not interpolated)", count, rows, m->C, m->cfg.image_size, m->grid, m->grid);
    }
    return ap::set_param(m, "clip_resnet", name, host, count);
}

int ap_clip_resnet_finalize(ap_clip_resnet* m) { return ap::finalize(m, "clip_resnet"); }

size_t ap_clip_resnet_workspace_bytes(const ap_clip_resnet* m, int n) {
    return m && n > 0 ? ap::Workspace4::bytes(m->max_act, n, m->cfg.compute_dtype) : 0;
}

int ap_clip_resnet_embed_dim(const ap_clip_resnet* m) { return m ? m->cfg.output_dim : 0; }

int ap_clip_resnet_profile_enable(ap_clip_resnet* m, int on) { return ap::profile_enable(m ? &m->prof : nullptr, "clip_resnet", on); }

int ap_clip_resnet_profile_read(ap_clip_resnet* m, double* ms_by_kind, long long* launches_by_kind, int kinds) {
    return ap::profile_read(m ? &m->prof : nullptr, "clip_resnet", AP_CLIP_RESNET_PROF_KINDS, ms_by_kind, launches_by_kind, kinds);
}

int ap_clip_resnet_forward_u8(ap_clip_resnet* m, const uint8_t* patches, int n, int h, int w, const float mean[3],
                              const float stdv[3], float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream) {
    int rc = ap::check_forward_args("clip_resnet", m, n, patches && out && mean && stdv, workspace, workspace_bytes,
                                    ap_clip_resnet_workspace_bytes);
    if (rc != AP_OK || n == 0) return rc;
    const int S = m->cfg.image_size;
    AP_REQUIRE(h >= S && w >= S, "clip_resnet_forward_u8: %dx%d tiles smaller than the %d model input", h, w, S);
    hipStream_t s = (hipStream_t)stream;
    const int dt = m->cfg.compute_dtype;
    ap::Workspace4 ws(workspace, m->max_act, n, dt);
    char* const* buf = ws.buf;
    const int* f = ws.f;

    { ScopedTimer t(m->prof, AP_CLIP_RESNET_PROF_STEM, s);
      rc = ap::launch_preproc_nhwc8(patches, n, h, w, ap::center_crop_offset(h, S), ap::center_crop_offset(w, S), S, mean, stdv,
                                    buf[0], dt, s); }
    if (rc != AP_OK) return rc;
    int hw = S / 2;
    if ((rc = run_conv(m, AP_CLIP_RESNET_PROF_STEM, m->stem[0], buf[0], n, S, nullptr, 1, buf[1], s)) != AP_OK) return rc;
    if ((rc = run_conv(m, AP_CLIP_RESNET_PROF_STEM, m->stem[1], buf[1], n, hw, nullptr, 1, buf[2], s)) != AP_OK) return rc;
    if ((rc = run_conv(m, AP_CLIP_RESNET_PROF_STEM, m->stem[2], buf[2], n, hw, nullptr, 1, buf[1], s)) != AP_OK) return rc;
    if ((rc = run_pool(m, buf[1], n, hw, m->stem[2].w->cout_stored, buf[2], s)) != AP_OK) return rc;
    hw /= 2;
    int xi = 2;                                     // buffer holding the current activation
    for (const Block& b : m->blocks) {
        ws.others(xi);
        const void* x = buf[xi];
        const int cin = b.c1.w->cin_stored, planes = b.c2.w->cout_stored;
        if ((rc = run_conv(m, conv_kind(b.c1), b.c1, x, n, hw, nullptr, 1, buf[f[0]], s)) != AP_OK) return rc;
        if ((rc = run_conv(m, conv_kind(b.c2), b.c2, buf[f[0]], n, hw, nullptr, 1, buf[f[1]], s)) != AP_OK) return rc;
        int oi;
        if (b.stride == 2) {
            const int ho = hw / 2;
            if ((rc = run_pool(m, x, n, hw, cin, buf[f[0]], s)) != AP_OK) return rc;
            if ((rc = run_conv(m, conv_kind(b.down), b.down, buf[f[0]], n, ho, nullptr, 0, buf[f[2]], s)) != AP_OK) return rc;
            if ((rc = run_pool(m, buf[f[1]], n, hw, planes, buf[f[0]], s)) != AP_OK) return rc;
            oi = f[1];
            if ((rc = run_conv(m, conv_kind(b.c3), b.c3, buf[f[0]], n, ho, buf[f[2]], 1, buf[oi], s)) != AP_OK) return rc;
            hw = ho;
        } else {
            const void* sc = x;
            if (b.down.w) {
                if ((rc = run_conv(m, conv_kind(b.down), b.down, x, n, hw, nullptr, 0, buf[f[2]], s)) != AP_OK) return rc;
                sc = buf[f[2]];
            }
            oi = f[0];
            if ((rc = run_conv(m, conv_kind(b.c3), b.c3, buf[f[1]], n, hw, sc, 1, buf[oi], s)) != AP_OK) return rc;
        }
        xi = oi;
    }

    // ---- attention-pool head
    ws.others(xi);
    const int C = m->C, tokens = hw * hw + 1, D = m->cfg.output_dim;
    ScopedTimer t(m->prof, AP_CLIP_RESNET_PROF_HEAD, s);
    rc = ap::launch_clip_attnpool_tokens(dt, buf[xi], (const float*)m->pos->d, n, hw * hw, C, buf[f[0]], buf[f[1]], s);
    if (rc != AP_OK) return rc;
    rc = ap::launch_conv2d_nhwc(dt, buf[f[0]], n * tokens, 1, 1, C, m->kv.w->d, (const float*)m->kv.b->d, 2 * C, 1, 1, 0, nullptr, 0,
                                buf[f[2]], s);
    if (rc != AP_OK) return rc;
    rc = ap::launch_conv2d_nhwc(dt, buf[f[1]], n, 1, 1, C, m->q.w->d, (const float*)m->q.b->d, C, 1, 1, 0, nullptr, 0, buf[xi], s);
    if (rc != AP_OK) return rc;
    rc = ap::launch_attention_cls(dt, buf[xi], buf[f[2]], 2 * C, 0, C, buf[f[0]], n, tokens, C / HEAD_DIM, HEAD_DIM, 0.125f, s);
    if (rc != AP_OK) return rc;
    const bool f32 = dt == AP_F32 && ((uintptr_t)out & 15) == 0;            // float32: c_proj writes the caller's buffer itself
    void* feat = f32 ? (void*)out : (void*)buf[f[1]];
    rc = ap::launch_conv2d_nhwc_ex(dt, buf[f[0]], n, 1, 1, C, m->cproj.w->d, (const float*)m->cproj.b->d, D, 1, 1, 0, nullptr, 0, feat, s);
    if (rc != AP_OK || f32) return rc;
    if (dt == AP_F32) {
        AP_HIP_CHECK(hipMemcpyAsync(out, feat, (size_t)n * D * sizeof(float), hipMemcpyDeviceToDevice, s));
        return AP_OK;
    }
    return ap::launch_stream_to_f32(dt, feat, D, n, D, out, s);
}

}  // extern "C"
