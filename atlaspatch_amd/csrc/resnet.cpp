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
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "ap_common.h"

namespace {

struct ConvParam {
    int cout = 0, cin = 0, cin_stored = 0, ks = 0;
    void* w = nullptr;          // T [cout][ks][ks][cin_stored]
    float* b = nullptr;         // f32 [cout]
    bool w_set = false, b_set = false;
};

struct ConvOp {                 // one convolution of the forward, resolved at create
    ConvParam* p;
    int stride, pad;
};

struct Block {
    ConvOp c1, c2, c3;          // c3 unused for basic blocks
    ConvOp down;                // down.p == nullptr: identity shortcut
};

}  // namespace

struct ap_resnet {
    ap_resnet_config cfg;
    std::map<std::string, ConvParam> params;
    ConvOp stem{};
    std::vector<Block> blocks;
    int out_dim = 0;
    size_t max_act = 0;         // elements per image of the largest activation
    bool finalized = false;
    bool profile = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_used;
    size_t ev_next = 0;
};

namespace {

hipEvent_t next_event(ap_resnet* m) {
    if (m->ev_next == m->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        m->ev_pool.push_back(e);
    }
    return m->ev_pool[m->ev_next++];
}
struct ScopedTimer {      // records start/stop events around one launch when profiling is on
    ap_resnet* m; int kind; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(ap_resnet* m_, int kind_, hipStream_t s_) : m(m_), kind(kind_), s(s_) {
        if (m->profile) { a = next_event(m); b = next_event(m); if (a) (void)hipEventRecord(a, s); }
    }
    ~ScopedTimer() {
        if (m->profile && a && b) { (void)hipEventRecord(b, s); m->ev_used.push_back({kind, {a, b}}); }
    }
};

int add_conv(ap_resnet* m, const std::string& name, int cout, int cin, int ks, int stride, ConvOp* op) {
    ConvParam p;
    p.cout = cout; p.cin = cin; p.cin_stored = (int)ap::align_up(cin, 8); p.ks = ks;
    const size_t wbytes = (size_t)cout * ks * ks * p.cin_stored * ap::dtype_size(m->cfg.compute_dtype);
    AP_HIP_CHECK(hipMalloc(&p.w, wbytes));
    AP_HIP_CHECK(hipMemset(p.w, 0, wbytes));
    AP_HIP_CHECK(hipMalloc((void**)&p.b, (size_t)cout * sizeof(float)));
    m->params[name] = p;
    op->p = &m->params[name];        // std::map nodes are stable
    op->stride = stride;
    op->pad = ks / 2;
    return AP_OK;
}

void free_params(ap_resnet* m) {
    for (auto& kv : m->params) {
        if (kv.second.w) (void)hipFree(kv.second.w);
        if (kv.second.b) (void)hipFree(kv.second.b);
    }
    m->params.clear();
}

size_t align256(size_t v) { return ap::align_up(v, 256); }

int run_conv(ap_resnet* m, const ConvOp& op, const void* x, int n, int h, int w, const void* resid, int relu, void* out,
             hipStream_t s) {
    const int kind = op.p->ks == 7 ? AP_RESNET_PROF_STEM : (op.p->ks == 1 ? AP_RESNET_PROF_CONV1X1 : AP_RESNET_PROF_CONV3X3);
    ScopedTimer t(m, kind, s);
    return ap::launch_conv2d_nhwc(m->cfg.compute_dtype, x, n, h, w, op.p->cin_stored, op.p->w, op.p->b, op.p->cout, op.p->ks,
                                  op.stride, op.pad, resid, relu, out, s);
}

inline int conv_out(int h, const ConvOp& op) { return (h + 2 * op.pad - op.p->ks) / op.stride + 1; }

}  // namespace

extern "C" {

size_t ap_sizeof_resnet_config(void) { return sizeof(ap_resnet_config); }

int ap_resnet_config_init(ap_resnet_config* cfg, size_t sizeof_caller) {
    AP_REQUIRE(cfg, "resnet_config_init: null argument");
    AP_REQUIRE(sizeof_caller >= AP_RESNET_CONFIG_SIZE_V20 && sizeof_caller % 4 == 0 && sizeof_caller <= 4096,
               "resnet_config_init: %zu is not the size of an ap_resnet_config (%u bytes, this library: %zu)", sizeof_caller,
               AP_RESNET_CONFIG_SIZE_V20, sizeof(ap_resnet_config));
    memset(cfg, 0, sizeof_caller);
    cfg->struct_size = (uint32_t)sizeof_caller;
    return AP_OK;
}

int ap_resnet_create(const ap_resnet_config* cfg, ap_resnet** out) {
    AP_REQUIRE(cfg && out, "resnet_create: null argument");
    static_assert(sizeof(ap_resnet_config) == AP_RESNET_CONFIG_SIZE_V20, "ap_resnet_config grew: append only, list the sizes it has had");
    const size_t given = cfg->struct_size;
    if (given > sizeof(ap_resnet_config) && given % 4 == 0 && given <= 4096) {
        ap::set_error("resnet_create: cfg->struct_size = %zu is larger than this library's ap_resnet_config (%zu bytes): the binding "
                      "was generated from a newer include/atlaspatch_hip.h than the library was built from", given, sizeof(ap_resnet_config));
        return AP_ERR_UNSUPPORTED;
    }
    AP_REQUIRE(given == AP_RESNET_CONFIG_SIZE_V20,
               "resnet_create: cfg->struct_size = %zu is not a size ap_resnet_config has had (%u bytes): fill the structure with "
               "ap_resnet_config_init(&cfg, sizeof cfg)", given, AP_RESNET_CONFIG_SIZE_V20);
    ap_resnet_config c;
    memcpy(&c, cfg, sizeof(c));
    AP_REQUIRE(c.block == AP_RESNET_BASIC || c.block == AP_RESNET_BOTTLENECK, "resnet_create: block %d", c.block);
    for (int s = 0; s < 4; ++s) AP_REQUIRE(c.depths[s] >= 1 && c.depths[s] <= 64, "resnet_create: depths[%d] = %d", s, c.depths[s]);
    AP_REQUIRE(c.stem_width >= 64 && c.stem_width % 64 == 0 && c.stem_width <= 256, "resnet_create: stem_width %d (a multiple of 64)",
               c.stem_width);
    AP_REQUIRE(c.compute_dtype == AP_F16 || c.compute_dtype == AP_BF16 || c.compute_dtype == AP_F32,
               "resnet_create: compute dtype %d", c.compute_dtype);
    AP_REQUIRE(c.image_size >= 32 && c.image_size <= 1024, "resnet_create: image_size %d", c.image_size);
    ap_resnet* m = new ap_resnet();
    m->cfg = c;
    int rc = AP_OK;
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
    if (rc != AP_OK) { ap_resnet_destroy(m); return rc; }
    *out = m;
    return AP_OK;
}

void ap_resnet_destroy(ap_resnet* m) {
    if (!m) return;
    free_params(m);
    for (hipEvent_t e : m->ev_pool) (void)hipEventDestroy(e);
    delete m;
}

int ap_resnet_set_param(ap_resnet* m, const char* name, const float* host, size_t count) {
    AP_REQUIRE(m && name && host, "resnet_set_param: null argument");
    std::string key(name);
    const bool is_w = key.size() > 7 && key.compare(key.size() - 7, 7, ".weight") == 0;
    const bool is_b = key.size() > 5 && key.compare(key.size() - 5, 5, ".bias") == 0;
    AP_REQUIRE(is_w || is_b, "resnet_set_param: unknown parameter '%s'", name);
    const std::string base = key.substr(0, key.size() - (is_w ? 7 : 5));
    auto it = m->params.find(base);
    AP_REQUIRE(it != m->params.end(), "resnet_set_param: unknown parameter '%s'", name);
    ConvParam& p = it->second;
    if (is_b) {
        AP_REQUIRE(count == (size_t)p.cout, "resnet_set_param: %s has %zu values, expected %d", name, count, p.cout);
        AP_HIP_CHECK(hipMemcpy(p.b, host, count * sizeof(float), hipMemcpyHostToDevice));
        p.b_set = true;
    } else {
        const size_t want = (size_t)p.cout * p.cin * p.ks * p.ks;
        AP_REQUIRE(count == want, "resnet_set_param: %s has %zu values, expected %zu ([%d, %d, %d, %d])", name, count, want, p.cout,
                   p.cin, p.ks, p.ks);
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
            ap::set_error("resnet_set_param: hipMemcpy of %s failed", name);
            rc = AP_ERR_HIP;
        }
        if (rc == AP_OK) rc = ap::launch_convert(m->cfg.compute_dtype, tmp, p.w, elems, nullptr);
        if (rc == AP_OK && hipDeviceSynchronize() != hipSuccess) {
            ap::set_error("resnet_set_param: conversion of %s failed", name);
            rc = AP_ERR_HIP;
        }
        (void)hipFree(tmp);
        if (rc != AP_OK) return rc;
        p.w_set = true;
    }
    m->finalized = false;
    return AP_OK;
}

int ap_resnet_finalize(ap_resnet* m) {
    AP_REQUIRE(m, "resnet_finalize: null handle");
    for (auto& kv : m->params) {
        if (!kv.second.w_set || !kv.second.b_set) {
            ap::set_error("resnet_finalize: parameter '%s.%s' was never set", kv.first.c_str(), kv.second.w_set ? "bias" : "weight");
            return AP_ERR_STATE;
        }
    }
    m->finalized = true;
    return AP_OK;
}

size_t ap_resnet_workspace_bytes(const ap_resnet* m, int n) {
    if (!m || n <= 0) return 0;
    return 4 * align256(m->max_act * (size_t)n * ap::dtype_size(m->cfg.compute_dtype));
}

int ap_resnet_embed_dim(const ap_resnet* m) { return m ? m->out_dim : 0; }

int ap_resnet_profile_enable(ap_resnet* m, int on) {
    AP_REQUIRE(m, "resnet_profile_enable: null handle");
    m->profile = on != 0;
    m->ev_used.clear();
    m->ev_next = 0;
    return AP_OK;
}

int ap_resnet_profile_read(ap_resnet* m, double* ms_by_kind, long long* launches_by_kind, int kinds) {
    AP_REQUIRE(m && ms_by_kind && launches_by_kind && kinds >= AP_RESNET_PROF_KINDS, "resnet_profile_read: bad arguments");
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

int ap_resnet_forward_u8(ap_resnet* m, const uint8_t* patches, int n, int h, int w, const float mean[3], const float stdv[3],
                         float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream) {
    AP_REQUIRE(m != nullptr, "resnet: null handle");
    if (!m->finalized) { ap::set_error("resnet: ap_resnet_finalize has not been called"); return AP_ERR_STATE; }
    AP_REQUIRE(n >= 0, "resnet: negative batch");
    if (n == 0) return AP_OK;
    AP_REQUIRE(patches && out && workspace && mean && stdv, "resnet: null buffer");
    AP_REQUIRE(((uintptr_t)workspace & 255) == 0, "resnet: workspace must be 256-byte aligned");
    if (workspace_bytes < ap_resnet_workspace_bytes(m, n)) {
        ap::set_error("resnet: workspace %zu bytes < required %zu", workspace_bytes, ap_resnet_workspace_bytes(m, n));
        return AP_ERR_WORKSPACE;
    }
    const int S = m->cfg.image_size;
    AP_REQUIRE(h >= S && w >= S, "resnet_forward_u8: %dx%d tiles smaller than the %d model input", h, w, S);
    // torchvision CenterCrop: top = int(round((h - S) / 2.0)) (banker's rounding), as ap_vit_forward_u8
    auto crop_off = [](int full, int size) { int d = full - size; return (d / 2) + ((d & 1) && ((d / 2) & 1) ? 1 : 0); };
    hipStream_t s = (hipStream_t)stream;
    const int dt = m->cfg.compute_dtype;
    const size_t slot = align256(m->max_act * (size_t)n * ap::dtype_size(dt));
    char* buf[4];
    for (int i = 0; i < 4; ++i) buf[i] = (char*)workspace + i * slot;

    int rc;
    { ScopedTimer t(m, AP_RESNET_PROF_STEM, s);
      rc = ap::launch_preproc_nhwc8(patches, n, h, w, crop_off(h, S), crop_off(w, S), S, mean, stdv, buf[0], dt, s); }
    if (rc != AP_OK) return rc;
    rc = run_conv(m, m->stem, buf[0], n, S, S, nullptr, 1, buf[1], s);
    if (rc != AP_OK) return rc;
    int hw = conv_out(S, m->stem);
    { ScopedTimer t(m, AP_RESNET_PROF_POOL, s);
      rc = ap::launch_maxpool3x3s2_nhwc(dt, buf[1], n, hw, hw, m->stem.p->cout, buf[2], s); }
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
        if (b.down.p) {
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
    { ScopedTimer t(m, AP_RESNET_PROF_POOL, s);
      rc = ap::launch_avgpool_nhwc(dt, buf[xi], n, hw * hw, m->out_dim, out, s); }
    return rc;
}

}  // extern "C"
