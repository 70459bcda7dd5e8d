// Host part shared by the two ResNet engines (resnet.cpp: torchvision, clip_resnet.cpp: OpenAI CLIP): the convolution and
// block records, the walk over the four stages that registers their parameters, the launch of one convolution and the
// four-buffer workspace.  Host C++ only; the two forwards stay in their own files, they are different launch sequences.
#pragma once
#include <algorithm>
#include <string>
#include <vector>
#include "engine_host.h"

namespace ap {

struct ConvOp : Conv {          // one convolution of the forward; padding ks / 2
    int stride = 1;
};

struct Block {
    ConvOp c1, c2, c3;          // c3.w == nullptr: a basic block (two 3x3 convolutions)
    ConvOp down;                // down.w == nullptr: identity shortcut
    int stride = 1;
};

inline int padded32(int c) { return (int)align_up((size_t)c, 32); }

struct StagePlan {
    bool bottleneck;            // 1x1, 3x3, 1x1 with expansion 4; else two 3x3
    int width;                  // planes of stage s: width << s
    const int* depths;          // blocks of the four stages
    bool pad32;                 // maps are stored with their channels rounded up to 32 (else as they are)
    bool stride_in_conv;        // a block's stride sits in its 3x3 convolution and its projection; else the engine pools 2x2
                                // behind the 3x3 convolution and in front of the projection, and every convolution has stride 1
};

struct Stages {
    std::vector<Block> blocks;
    int channels = 0, hw = 0;   // the final map: hw x hw pixels of `channels` channels
    size_t max_act = 0;         // elements per image of the largest tensor a block reads or writes
};

// Registers "layer<S>.<B>.conv<K>" / "layer<S>.<B>.downsample" (.weight, .bias) of every block; the first block of stages 2..4
// has stride 2, and a block whose stride or channel count changes has a projection.  (inplanes, hw): the map the first block reads.
inline int add_stages(ParamStore& store, const StagePlan& plan, int inplanes, int hw, Stages* out) {
    auto stored = [&](int c) { return plan.pad32 ? padded32(c) : c; };
    int rc = AP_OK;
    auto add = [&](const std::string& name, int cout, int cin, int ks, int stride, ConvOp* op) {
        op->stride = plan.stride_in_conv ? stride : 1;
        if (rc == AP_OK) rc = add_conv(store, name, cout, cin, ks, stored(cout), stored(cin), op);
    };
    for (int s = 0; s < 4; ++s) {
        const int planes = plan.width << s, outc = plan.bottleneck ? planes * 4 : planes;
        for (int b = 0; b < plan.depths[s]; ++b) {
            const std::string pre = "layer" + std::to_string(s + 1) + "." + std::to_string(b) + ".";
            Block blk{};
            blk.stride = (s > 0 && b == 0) ? 2 : 1;
            const int ho = (hw - 1) / blk.stride + 1;
            if (plan.bottleneck) {
                add(pre + "conv1", planes, inplanes, 1, 1, &blk.c1);
                add(pre + "conv2", planes, planes, 3, blk.stride, &blk.c2);
                add(pre + "conv3", outc, planes, 1, 1, &blk.c3);
            } else {
                add(pre + "conv1", planes, inplanes, 3, blk.stride, &blk.c1);
                add(pre + "conv2", planes, planes, 3, 1, &blk.c2);
            }
            if (blk.stride != 1 || inplanes != outc) add(pre + "downsample", outc, inplanes, 1, blk.stride, &blk.down);
            // the block's input, conv1's output (a bottleneck's: still at the input's size; conv2's and the pooled maps are no
            // larger), and the outputs of the last convolution and the projection
            const int hmid = plan.bottleneck ? hw : ho;
            out->max_act = std::max({out->max_act, (size_t)hw * hw * stored(inplanes), (size_t)hmid * hmid * stored(planes),
                                     (size_t)ho * ho * stored(outc)});
            hw = ho;
            inplanes = outc;
            out->blocks.push_back(blk);
        }
    }
    out->channels = inplanes;
    out->hw = hw;
    return rc;
}

// x T [n, h, w, cin_stored] -> out T [n, ho, wo, cout_stored] = act(conv + bias (+ resid)).  A stored Cout that is a multiple
// of 64 takes the plain kernel, any other (32 mod 64) the _ex form: two different code objects.
inline int run_conv(LaunchProfiler& prof, int kind, int dtype, const ConvOp& op, const void* x, int n, int h, int w,
                    const void* resid, int relu, void* out, hipStream_t s) {
    const DevParam& p = *op.w;
    ScopedTimer t(prof, kind, s);
    const auto launch = p.cout_stored % 64 == 0 ? launch_conv2d_nhwc : launch_conv2d_nhwc_ex;
    return launch(dtype, x, n, h, w, p.cin_stored, p.d, (const float*)op.b->d, p.cout_stored, p.ks, op.stride, p.ks / 2, resid, relu,
                  out, s);
}

// ---- workspace: four buffers of the largest activation each, rotated so that no launch writes a buffer it reads
struct Workspace4 {
    char* buf[4];
    int f[3];                   // the three buffers other than `xi`, ascending (others())

    static size_t slot_bytes(size_t max_act, int n, int dtype) { return align_up(max_act * (size_t)n * dtype_size(dtype), 256); }
    static size_t bytes(size_t max_act, int n, int dtype) { return 4 * slot_bytes(max_act, n, dtype); }

    Workspace4(void* workspace, size_t max_act, int n, int dtype) {
        const size_t slot = slot_bytes(max_act, n, dtype);
        for (int i = 0; i < 4; ++i) buf[i] = (char*)workspace + i * slot;
    }
    void others(int xi) {
        int k = 0;
        for (int i = 0; i < 4; ++i) if (i != xi) f[k++] = i;
    }
};

}  // namespace ap
