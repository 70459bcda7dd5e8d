// ResNet encoder object behind the C ABI (ap_resnet_*): parameter storage in HBM, workspace carving and the launch sequence
// of one forward pass.  Host C++ only; every kernel it launches lives in conv.hip, and the block records, the stage walk, the
// convolution launch and the four-buffer workspace are resnet_host.h's, shared with clip_resnet.cpp.
//
// Forward for n images (T = compute dtype, NHWC everywhere):
//   preprocess  u8 tiles -> centre crop -> normalised T [n, S, S, 8] (channels 3..7 zero)
//   stem        conv 7x7 s2 p3 (+ folded BN, ReLU) -> [n, S/2, S/2, W]; max pool 3x3 s2 p1 -> [n, S/4, S/4, W]
//   stages      torchvision BasicBlock / Bottleneck (stride on the 3x3 conv); each conv carries its folded BatchNorm as a
//               bias, the block's last conv adds the shortcut (identity or the 1x1 projection + BN) and applies ReLU
//   head        global average pool -> f32 [n, C]
// Workspace: four buffers of the largest activation each (the stem input included), rotated so that a block never writes a
// buffer it still reads: x (input) -> t1 -> t2 (-> projection) -> out, out becomes the next block's x.
#include "resnet_host.h"

using ap::Block;
using ap::ConvOp;
using ap::ScopedTimer;

struct ap_resnet {
    ap_resnet_config cfg;
    ap::ParamStore params;
    ConvOp stem;
    std::vector<Block> blocks;
    int out_dim = 0;
    size_t max_act = 0;         // elements per image of the largest activation
    bool finalized = false;
    ap::LaunchProfiler prof;
};

namespace {

int run_conv(ap_resnet* m, const ConvOp& op, const void* x, int n, int hw, const void* resid, int relu, void* out, hipStream_t s) {
    const int ks = op.w->ks;
    const int kind = ks == 7 ? AP_RESNET_PROF_STEM : (ks == 1 ? AP_RESNET_PROF_CONV1X1 : AP_RESNET_PROF_CONV3X3);
    return ap::run_conv(m->prof, kind, m->cfg.compute_dtype, op, x, n, hw, hw, resid, relu, out, s);
}

}  // namespace

extern "C" {

size_t ap_sizeof_resnet_config(void) { return sizeof(ap_resnet_config); }

int ap_resnet_config_init(ap_resnet_config* cfg, size_t sizeof_caller) {
    return ap::config_init("resnet", cfg, sizeof_caller, AP_RESNET_CONFIG_SIZE_V20);
}

int ap_resnet_create(const ap_resnet_config* cfg, ap_resnet** out) {
    AP_REQUIRE(cfg && out, "resnet_create: null argument");
    static_assert(sizeof(ap_resnet_config) == AP_RESNET_CONFIG_SIZE_V20, "ap_resnet_config grew: append only, list the sizes it has had");
    ap_resnet_config c;
    int rc = ap::accept_config("resnet", cfg, 4096, "", &c);
    if (rc != AP_OK) return rc;
    AP_REQUIRE(c.block == AP_RESNET_BASIC || c.block == AP_RESNET_BOTTLENECK, "resnet_create: block %d", c.block);
    for (int s = 0; s < 4; ++s) AP_REQUIRE(c.depths[s] >= 1 && c.depths[s] <= 64, "resnet_create: depths[%d] = %d", s, c.depths[s]);
    AP_REQUIRE(c.stem_width >= 64 && c.stem_width % 64 == 0 && c.stem_width <= 256, "resnet_create: stem_width %d (a multiple of 64)",
               c.stem_width);
    if ((rc = ap::check_compute_dtype("resnet", c.compute_dtype)) != AP_OK) return rc;
    AP_REQUIRE(c.image_size >= 32 && c.image_size <= 1024, "resnet_create: image_size %d", c.image_size);
    ap_resnet* m = new ap_resnet();
    m->cfg = c;
    m->params.dtype = c.compute_dtype;
    const int W = c.stem_width;
    m->stem.stride = 2;
    rc = ap::add_conv(m->params, "conv1", W, 3, 7, &m->stem);
    const int h1 = (c.image_size + 6 - 7) / 2 + 1;          // the stem convolution's map; the max pool halves it once more
    ap::Stages st;
    if (rc == AP_OK)
        rc = ap::add_stages(m->params, {c.block == AP_RESNET_BOTTLENECK, W, c.depths, false, true}, W, (h1 - 1) / 2 + 1, &st);
    m->blocks = std::move(st.blocks);
    m->out_dim = st.channels;
    m->max_act = std::max({(size_t)c.image_size * c.image_size * 8, (size_t)h1 * h1 * W, st.max_act});
    if (rc != AP_OK) { delete m; return rc; }
    *out = m;
    return AP_OK;
}

void ap_resnet_destroy(ap_resnet* m) { delete m; }

int ap_resnet_set_param(ap_resnet* m, const char* name, const float* host, size_t count) {
    return ap::set_param(m, "resnet", name, host, count);
}

int ap_resnet_finalize(ap_resnet* m) { return ap::finalize(m, "resnet"); }

size_t ap_resnet_workspace_bytes(const ap_resnet* m, int n) {
    return m && n > 0 ? ap::Workspace4::bytes(m->max_act, n, m->cfg.compute_dtype) : 0;
}

int ap_resnet_embed_dim(const ap_resnet* m) { return m ? m->out_dim : 0; }

int ap_resnet_profile_enable(ap_resnet* m, int on) { return ap::profile_enable(m ? &m->prof : nullptr, "resnet", on); }

int ap_resnet_profile_read(ap_resnet* m, double* ms_by_kind, long long* launches_by_kind, int kinds) {
    return ap::profile_read(m ? &m->prof : nullptr, "resnet", AP_RESNET_PROF_KINDS, ms_by_kind, launches_by_kind, kinds);
}

int ap_resnet_forward_u8(ap_resnet* m, const uint8_t* patches, int n, int h, int w, const float mean[3], const float stdv[3],
                         float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream) {
    int rc = ap::check_forward_args("resnet", m, n, patches && out && mean && stdv, workspace, workspace_bytes,
                                    ap_resnet_workspace_bytes);
    if (rc != AP_OK || n == 0) return rc;
    const int S = m->cfg.image_size;
    AP_REQUIRE(h >= S && w >= S, "resnet_forward_u8: %dx%d tiles smaller than the %d model input", h, w, S);
    hipStream_t s = (hipStream_t)stream;
    const int dt = m->cfg.compute_dtype;
    ap::Workspace4 ws(workspace, m->max_act, n, dt);
    char* const* buf = ws.buf;

    { ScopedTimer t(m->prof, AP_RESNET_PROF_STEM, s);
      rc = ap::launch_preproc_nhwc8(patches, n, h, w, ap::center_crop_offset(h, S), ap::center_crop_offset(w, S), S, mean, stdv,
                                    buf[0], dt, s); }
    if (rc != AP_OK) return rc;
    rc = run_conv(m, m->stem, buf[0], n, S, nullptr, 1, buf[1], s);
    if (rc != AP_OK) return rc;
    int hw = (S + 6 - 7) / 2 + 1;
    { ScopedTimer t(m->prof, AP_RESNET_PROF_POOL, s);
      rc = ap::launch_maxpool3x3s2_nhwc(dt, buf[1], n, hw, hw, m->stem.w->cout, buf[2], s); }
    if (rc != AP_OK) return rc;
    hw = (hw - 1) / 2 + 1;
    int xi = 2;                                     // buffer holding the current activation
    for (const Block& b : m->blocks) {
        ws.others(xi);
        const int* f = ws.f;
        const void* x = buf[xi];
        const int ho = (hw - 1) / b.stride + 1;
        const void* sc = x;
        if (b.down.w) {
            rc = run_conv(m, b.down, x, n, hw, nullptr, 0, buf[f[2]], s);
            if (rc != AP_OK) return rc;
            sc = buf[f[2]];
        }
        int oi;
        if (b.c3.w) {
            // x -> t1 (f0) -> t2 (f1) -> out (f0, t1 is dead once t2 exists); shortcut in f2 or x
            if ((rc = run_conv(m, b.c1, x, n, hw, nullptr, 1, buf[f[0]], s)) != AP_OK) return rc;
            if ((rc = run_conv(m, b.c2, buf[f[0]], n, hw, nullptr, 1, buf[f[1]], s)) != AP_OK) return rc;
            oi = f[0];
            if ((rc = run_conv(m, b.c3, buf[f[1]], n, ho, sc, 1, buf[oi], s)) != AP_OK) return rc;
        } else {
            // x -> t1 (f0) -> out (f1); shortcut in f2 or x
            if ((rc = run_conv(m, b.c1, x, n, hw, nullptr, 1, buf[f[0]], s)) != AP_OK) return rc;
            oi = f[1];
            if ((rc = run_conv(m, b.c2, buf[f[0]], n, ho, sc, 1, buf[oi], s)) != AP_OK) return rc;
        }
        xi = oi;
        hw = ho;
    }
    { ScopedTimer t(m->prof, AP_RESNET_PROF_POOL, s);
      rc = ap::launch_avgpool_nhwc(dt, buf[xi], n, hw * hw, m->out_dim, out, s); }
    return rc;
}

}  // extern "C"
