// ResNet encoder object behind the C ABI (ap_resnet_*): parameter storage in HBM, workspace carving and the launch sequence
// of one forward pass.  Host C++ only; every kernel it launches lives in conv.hip.
//
// Forward for n images (T = compute dtype, NHWC everywhere):
//   preprocess  u8 tiles -> centre crop -> normalised T [n, S, S, 8] (channels 3..7 zero)
//   stem        conv 7x7 s2 p3 (+ folded BN, ReLU) -> [n, S/2, S/2, W]; max pool 3x3 s2 p1 -> [n, S/4, S/4, W]
//   stages      torchvision BasicBlock / Bottleneck (stride on the 3x3 conv); each conv carries its folded BatchNorm as a
//               bias, the block's last conv adds the shortcut (identity or the 1x1 projection + BN) and applies ReLU
//   head        global average pool -> f32 [n, C]
// Workspace: four buffers of the largest activation each (the stem input included), rotated so that a block never writes a
// buffer it still reads: x (input) -> t1 -> t2 (-> projection) -> out, out becomes the next block's x.
#include <algorithm>
#include <string>
#include <vector>
#include "engine_host.h"

namespace {

using ap::DevParam;
using ap::ScopedTimer;

struct ConvOp {                 // one convolution of the forward, resolved at create
    DevParam* w = nullptr;      // "<conv>.weight": T [cout][ks][ks][cin_stored]
    DevParam* b = nullptr;      // "<conv>.bias": f32 [cout]
    int stride = 1, pad = 0;
};

struct Block {
    ConvOp c1, c2, c3;          // c3 unused for basic blocks
    ConvOp down;                // down.w == nullptr: identity shortcut
};

}  // namespace

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

int add_conv(ap_resnet* m, const std::string& name, int cout, int cin, int ks, int stride, ConvOp* op) {
    op->stride = stride;
    op->pad = ks / 2;
    const int rc = m->params.add(name + ".weight", ap::P_CONV_W, cout, cin, ks, &op->w);
    return rc != AP_OK ? rc : m->params.add(name + ".bias", ap::P_VEC, cout, 0, 0, &op->b);
}

size_t align256(size_t v) { return ap::align_up(v, 256); }

int run_conv(ap_resnet* m, const ConvOp& op, const void* x, int n, int h, int w, const void* resid, int relu, void* out,
             hipStream_t s) {
    const DevParam& p = *op.w;
    const int kind = p.ks == 7 ? AP_RESNET_PROF_STEM : (p.ks == 1 ? AP_RESNET_PROF_CONV1X1 : AP_RESNET_PROF_CONV3X3);
    ScopedTimer t(m->prof, kind, s);
    return ap::launch_conv2d_nhwc(m->cfg.compute_dtype, x, n, h, w, p.cin_stored, p.d, (const float*)op.b->d, p.cout, p.ks,
                                  op.stride, op.pad, resid, relu, out, s);
}

inline int conv_out(int h, const ConvOp& op) { return (h + 2 * op.pad - op.w->ks) / op.stride + 1; }

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
    AP_REQUIRE(c.compute_dtype == AP_F16 || c.compute_dtype == AP_BF16 || c.compute_dtype == AP_F32,
               "resnet_create: compute dtype %d", c.compute_dtype);
    AP_REQUIRE(c.image_size >= 32 && c.image_size <= 1024, "resnet_create: image_size %d", c.image_size);
    ap_resnet* m = new ap_resnet();
    m->cfg = c;
    m->params.dtype = c.compute_dtype;
    auto add = [&](const std::string& name, int cout, int cin, int ks, int stride, ConvOp* op) {
        if (rc == AP_OK) rc = add_conv(m, name, cout, cin, ks, stride, op);
    };
    const int W = c.stem_width, expansion = c.block == AP_RESNET_BOTTLENECK ? 4 : 1;
    add("conv1", W, 3, 7, 2, &m->stem);
    int hw = c.image_size;
    size_t max_act = (size_t)hw * hw * 8;
    hw = (hw + 6 - 7) / 2 + 1;
    max_act = std::max(max_act, (size_t)hw * hw * W);
    hw = (hw - 1) / 2 + 1;
    int inplanes = W;
    for (int s = 0; s < 4; ++s) {
        const int planes = W << s, outc = planes * expansion;
        for (int b = 0; b < c.depths[s]; ++b) {
            const int stride = (s > 0 && b == 0) ? 2 : 1;
            const std::string pre = "layer" + std::to_string(s + 1) + "." + std::to_string(b) + ".";
            Block blk{};
            if (c.block == AP_RESNET_BOTTLENECK) {
                add(pre + "conv1", planes, inplanes, 1, 1, &blk.c1);
                add(pre + "conv2", planes, planes, 3, stride, &blk.c2);
                add(pre + "conv3", outc, planes, 1, 1, &blk.c3);
                max_act = std::max(max_act, (size_t)hw * hw * planes);
            } else {
                add(pre + "conv1", planes, inplanes, 3, stride, &blk.c1);
                add(pre + "conv2", planes, planes, 3, 1, &blk.c2);
            }
            if (stride != 1 || inplanes != outc) add(pre + "downsample", outc, inplanes, 1, stride, &blk.down);
            hw = (hw - 1) / stride + 1;
            max_act = std::max(max_act, (size_t)hw * hw * (size_t)std::max(outc, planes));
            inplanes = outc;
            m->blocks.push_back(blk);
        }
    }
    m->out_dim = inplanes;
    m->max_act = max_act;
    if (rc != AP_OK) { delete m; return rc; }
    *out = m;
    return AP_OK;
}

void ap_resnet_destroy(ap_resnet* m) { delete m; }

int ap_resnet_set_param(ap_resnet* m, const char* name, const float* host, size_t count) {
    AP_REQUIRE(m && name && host, "resnet_set_param: null argument");
    const int rc = m->params.set("resnet", name, host, count);
    if (rc == AP_OK) m->finalized = false;
    return rc;
}

int ap_resnet_finalize(ap_resnet* m) {
    AP_REQUIRE(m, "resnet_finalize: null handle");
    const int rc = m->params.check_all_set("resnet");
    if (rc == AP_OK) m->finalized = true;
    return rc;
}

size_t ap_resnet_workspace_bytes(const ap_resnet* m, int n) {
    if (!m || n <= 0) return 0;
    return 4 * align256(m->max_act * (size_t)n * ap::dtype_size(m->cfg.compute_dtype));
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
    const size_t slot = align256(m->max_act * (size_t)n * ap::dtype_size(dt));
    char* buf[4];
    for (int i = 0; i < 4; ++i) buf[i] = (char*)workspace + i * slot;

    { ScopedTimer t(m->prof, AP_RESNET_PROF_STEM, s);
      rc = ap::launch_preproc_nhwc8(patches, n, h, w, ap::center_crop_offset(h, S), ap::center_crop_offset(w, S), S, mean, stdv,
                                    buf[0], dt, s); }
    if (rc != AP_OK) return rc;
    rc = run_conv(m, m->stem, buf[0], n, S, S, nullptr, 1, buf[1], s);
    if (rc != AP_OK) return rc;
    int hw = conv_out(S, m->stem);
    { ScopedTimer t(m->prof, AP_RESNET_PROF_POOL, s);
      rc = ap::launch_maxpool3x3s2_nhwc(dt, buf[1], n, hw, hw, m->stem.w->cout, buf[2], s); }
    if (rc != AP_OK) return rc;
    hw = (hw - 1) / 2 + 1;
    int xi = 2;                                     // buffer holding the current activation
    for (const Block& b : m->blocks) {
        int f[3], k = 0;
        for (int i = 0; i < 4; ++i) if (i != xi) f[k++] = i;
        const void* x = buf[xi];
        const ConvOp& last = m->cfg.block == AP_RESNET_BOTTLENECK ? b.c3 : b.c2;
        const int stride = m->cfg.block == AP_RESNET_BOTTLENECK ? b.c2.stride : b.c1.stride;
        const int ho = (hw - 1) / stride + 1;
        const void* sc = x;
        if (b.down.w) {
            rc = run_conv(m, b.down, x, n, hw, hw, nullptr, 0, buf[f[2]], s);
            if (rc != AP_OK) return rc;
            sc = buf[f[2]];
        }
        int oi;
        if (m->cfg.block == AP_RESNET_BOTTLENECK) {
            // x -> t1 (f0) -> t2 (f1) -> out (f0, t1 is dead once t2 exists); shortcut in f2 or x
            if ((rc = run_conv(m, b.c1, x, n, hw, hw, nullptr, 1, buf[f[0]], s)) != AP_OK) return rc;
            if ((rc = run_conv(m, b.c2, buf[f[0]], n, hw, hw, nullptr, 1, buf[f[1]], s)) != AP_OK) return rc;
            oi = f[0];
            if ((rc = run_conv(m, last, buf[f[1]], n, ho, ho, sc, 1, buf[oi], s)) != AP_OK) return rc;
        } else {
            // x -> t1 (f0) -> out (f1); shortcut in f2 or x
            if ((rc = run_conv(m, b.c1, x, n, hw, hw, nullptr, 1, buf[f[0]], s)) != AP_OK) return rc;
            oi = f[1];
            if ((rc = run_conv(m, last, buf[f[0]], n, ho, ho, sc, 1, buf[oi], s)) != AP_OK) return rc;
        }
        xi = oi;
        hw = ho;
    }
    { ScopedTimer t(m->prof, AP_RESNET_PROF_POOL, s);
      rc = ap::launch_avgpool_nhwc(dt, buf[xi], n, hw * hw, m->out_dim, out, s); }
    return rc;
}

}  // extern "C"
