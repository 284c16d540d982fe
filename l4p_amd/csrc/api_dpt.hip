// l4p_dpt_forward: the whole DPT decoder of one dense head (reference DPTOutputAdapter_fix.forward,
// dpt_head.py:41-86 + dpt_block.py:93-157,210-238,255-278,406-414) as ONE native call: ~45 kernel launches
// issued back to back from C++ on the caller's stream, intermediates bump-allocated from a caller-provided
// workspace (graph.hpp).  This file is the one statement of the decoder's graph: every model forward, the benchmark and the
// tests run it, its dispatch switches are knobs (dpt_fold_rn, conv_ups), and l4p_amd/ops.py reaches the same kernels one by
// one for the per-kernel parity tests.
// One algebraic re-ordering against the reference: FeatureFusionBlock's out_conv (1x1x1) runs BEFORE the trilinear
// up-sampling instead of after it (dpt_block.py:229-237); both are linear and the interpolation weights sum to one.
// The allocator never releases here (the peak is the final offset); l4p_dpt_workspace_bytes is a dry run of run().
#include "gemm_select.hpp"
#include "graph.hpp"

namespace {

struct Vol {  // channels-last activation [B][t][h][w][c] of engine dtype
    void* p;
    int t, h, w, c;
    long long vox(int B) const { return (long long)B * t * h * w; }
};

struct Ctx : Graph {
    int B;
    Ctx(const l4p_engine* e_, int B_, std::string pre_ = std::string()) : Graph(e_, "l4p_dpt_forward", std::move(pre_)), B(B_) {}

    Vol vol(int t, int h, int w, int c) { return Vol{T((long long)B * t * h * w, c), t, h, w, c}; }

    // 1x1x1 conv: out = x @ w^T + bias on [vox][c] -> [vox][n]
    Vol conv1(const Vol& x, const char* wk, const char* bk, int n) {
        Vol o = vol(x.t, x.h, x.w, n);
        GemmParams p = dense(x.p, x.vox(B), x.c, x.c, W(wk), x.c, n);
        p.bias = Wf(bk);
        p.out_T = o.p, p.ldc = n;
        gemm(0, p);
        return o;
    }
    // ConvTranspose3d kernel == stride == k
    Vol convT(const Vol& x, const char* wk, const char* bk, int cout, const int k[3]) {
        Vol o = vol(x.t * k[0], x.h * k[1], x.w * k[2], cout);
        GemmParams p = dense(x.p, x.vox(B), x.c, x.c, W(wk), x.c, k[0] * k[1] * k[2] * cout);
        p.Ti = x.t, p.Hi = x.h, p.Wi = x.w;
        p.bias = Wf(bk);
        p.out_T = o.p;
        p.epi = EPI_CONVT;
        p.kt = k[0], p.kh = k[1], p.kw = k[2], p.Cout = cout;
        gemm(0, p);
        return o;
    }
    // ConvTranspose3d kernel == stride == k followed by the bias-free 3x3x3 conv, folded at pack time into one sub-pixel conv over
    // the low-resolution grid (l4p_conv3d_subpixel; weights fold{i}.w / fold{i}.b, packing.py fold_convT_rn)
    bool fold_fits(const Vol& x, const char* wk, const char* bk, int cout, const int k[3]) {
        // knob 1: levels whose three axes are all up-scaled (>= 8 sub-positions: a fifth to a third of the multiply-adds); 2: every
        // up-scaling level - the camray head's k = (2, 1, 1) keeps 2/3 of them and measured 85 + 150 us against 105 + 163 us per step
        const int kv = knob(KNOB_DPT_FOLD_RN);
        if (dry || !kv || (kv < 2 && k[0] * k[1] * k[2] < 8) || !e->find(pre + wk) || !e->find(pre + bk)) return false;
        return x.c % (128 / es) == 0 && cout % 128 == 0 && k[0] * k[1] * k[2] <= 64 && x.t * k[0] >= 2 && x.h * k[1] >= 2 && x.w * k[2] >= 2;
    }
    Vol fold(const Vol& x, const char* wk, const char* bk, int cout, const int k[3], Vol* relu_copy) {
        Vol o = vol(x.t * k[0], x.h * k[1], x.w * k[2], cout);
        if (relu_copy) *relu_copy = vol(o.t, o.h, o.w, cout);
        const int cells = (k[0] == 1 ? 3 : 2) * (k[1] == 1 ? 3 : 2) * (k[2] == 1 ? 3 : 2);
        GemmParams p = dense(x.p, x.vox(B), cells * x.c, 0, W(wk), (long long)cells * x.c, k[0] * k[1] * k[2] * cout);
        p.Ti = x.t, p.Hi = x.h, p.Wi = x.w, p.Cin = x.c;
        p.bias = Wf(bk);
        p.out_T = o.p;
        p.out_relu_T = relu_copy ? relu_copy->p : nullptr;
        p.kt = k[0], p.kh = k[1], p.kw = k[2], p.Cout = cout;
        gemm(2, p);
        return o;
    }
    // 3x3x3 conv, pad 1; optional bias / ReLU output / two T residuals / relu copy
    // ups_h / ups_w > 0: the conv reads x up-sampled (bilinear, align_corners) to ups_h x ups_w, formed in its loader
    Vol conv3(const Vol& x_in, const char* wk, const char* bk, int cout, const int s[3], int act, const void* r1, const void* r2,
              Vol* relu_copy, int ups_h = 0, int ups_w = 0) {
        Vol x = x_in;
        if (ups_h > 0) x.h = ups_h, x.w = ups_w;
        Vol o = vol((x.t - 1) / s[0] + 1, (x.h - 1) / s[1] + 1, (x.w - 1) / s[2] + 1, cout);
        if (relu_copy) *relu_copy = vol(o.t, o.h, o.w, cout);
        const long long M = o.vox(B);
        // (the caller of l4p_conv3d_k3 owns the split-K partials: l4p_conv3d_splitk is the rule for both sides)
        const int sk = ups_h > 0 ? 1 : conv3d_splitk(M, cout, 27 * x.c, es);
        float* partial = sk > 1 ? f32((long long)sk * M, cout) : nullptr;
        GemmParams p = dense(x.p, M, 27 * x.c, 0, W(wk), 27 * x.c, cout);
        p.Ti = x.t, p.Hi = x.h, p.Wi = x.w, p.Cin = x.c;
        p.To = o.t, p.Ho = o.h, p.Wo = o.w;
        p.st = s[0], p.sh = s[1], p.sw = s[2];
        p.bias = bk ? Wf(bk) : nullptr;
        p.act = act;
        if (r1) p.res1 = r1, p.res2 = r2, p.res_f32 = 0, p.ldr = cout;
        p.out_T = o.p, p.ldc = cout;
        p.out_relu_T = relu_copy ? relu_copy->p : nullptr;
        p.splitk = sk, p.partial = partial;
        if (ups_h > 0) p.ups_hi = x_in.h, p.ups_wi = x_in.w;
        gemm(1, p);
        return o;
    }
    Vol resize(const Vol& x, int t, int h, int w) {
        if (t == x.t && h == x.h && w == x.w) return x;
        Vol o = vol(t, h, w, x.c);
        launch([&] { return launch_upsample(dt, x.p, o.p, B, x.t, x.h, x.w, t, h, w, x.c, 1, st); });
        return o;
    }
};

int run(Ctx& c, const l4p_dpt_cfg* cfg, const void* const* hooks, float* out) {
    static const int one[3] = {1, 1, 1};
    const int F = cfg->feature_dim;
    Vol lay[4], layr[4];
    for (int i = 0; i < 4; ++i) {
        Vol tok{(void*)hooks[i], cfg->nt, cfg->nh, cfg->nw, cfg->dim};
        char wk[32], bk[32];
        snprintf(wk, sizeof(wk), "act%d.0.w", i);
        snprintf(bk, sizeof(bk), "act%d.0.b", i);
        Vol a = c.conv1(tok, wk, bk, cfg->layer_dims[i]);
        const int* sf = cfg->actpost[i];
        snprintf(wk, sizeof(wk), "act%d.1.w", i);
        snprintf(bk, sizeof(bk), "act%d.1.b", i);
        if (sf[0] > 0 || sf[1] > 0 || sf[2] > 0) {
            const int k[3] = {1 << sf[0], 1 << sf[1], 1 << sf[2]};
            // knob dpt_fold_rn: one sub-pixel conv in place of the two (the workspace is sized for the unfolded form, which needs
            // more: the knob may change between sizing and a forward)
            char fw[32], fb[32];
            snprintf(fw, sizeof(fw), "fold%d.w", i);
            snprintf(fb, sizeof(fb), "fold%d.b", i);
            if (c.fold_fits(a, fw, fb, F, k)) {
                lay[i] = c.fold(a, fw, fb, F, k, &layr[i]);
                continue;
            }
            a = c.convT(a, wk, bk, cfg->layer_dims[i], k);
        } else if (sf[0] < 0 || sf[1] < 0 || sf[2] < 0) {
            const int s[3] = {1 << -sf[0], 1 << -sf[1], 1 << -sf[2]};
            a = c.conv3(a, wk, bk, cfg->layer_dims[i], s, ACT_NONE, nullptr, nullptr, nullptr);
        }
        snprintf(wk, sizeof(wk), "rn%d.w", i);
        lay[i] = c.conv3(a, wk, nullptr, F, one, ACT_NONE, nullptr, nullptr, &layr[i]);
    }
    // ResidualConvUnit_custom (dpt_block.py:131-157): conv2(relu(conv1(relu(x)))) + x [+ extra].  relu(x) comes from the epilogue of
    // the kernel that produced x (so conv1 streams its input by LDS-DMA); conv1's own ReLU is an output activation; the skip adds
    // ride conv2's epilogue
    auto rcu = [&](int r, int u, const Vol& x, const Vol& xr, const void* extra, Vol* relu_copy) {
        char w1[40], b1[40], w2[40], b2[40];
        snprintf(w1, sizeof(w1), "ref%d.rcu%d.c1.w", r, u);
        snprintf(b1, sizeof(b1), "ref%d.rcu%d.c1.b", r, u);
        snprintf(w2, sizeof(w2), "ref%d.rcu%d.c2.w", r, u);
        snprintf(b2, sizeof(b2), "ref%d.rcu%d.c2.b", r, u);
        Vol y = c.conv3(xr, w1, b1, F, one, ACT_RELU, nullptr, nullptr, nullptr);
        return c.conv3(y, w2, b2, F, one, ACT_NONE, x.p, extra, relu_copy);
    };
    Vol path{};
    for (int r = 4; r >= 1; --r) {
        const int i = r - 1;
        Vol o, orl;
        if (r == 4) {
            o = lay[3];
            orl = layr[3];
        } else {
            Vol p4 = path;
            // dpt_head.py:70-72 crops refinenet4's output to layer 2's grid.  No geometry this engine is configured with reaches
            // that (token grids with an even number of frames and rows: the stride-2 level doubles back exactly): refused
            if (r == 3 && (p4.t != lay[2].t || p4.h != lay[2].h)) {
                l4p_set_error("l4p_dpt_forward: refinenet4 output needs cropping (unsupported token grid)");
                return L4P_E_INVALID;
            }
            o = rcu(r, 1, lay[i], layr[i], p4.p, &orl);  // path + RCU1(layer)
        }
        Vol o2 = rcu(r, 2, o, orl, nullptr, nullptr);
        char wk[32], bk[32];
        snprintf(wk, sizeof(wk), "ref%d.out.w", r);
        snprintf(bk, sizeof(bk), "ref%d.out.b", r);
        Vol oc = c.conv1(o2, wk, bk, F);  // out_conv commuted in front of the (linear) up-sampling
        const int* fs = cfg->fusion[i];
        path = c.resize(oc, oc.t * fs[0], oc.h * fs[1], oc.w * fs[2]);
    }
    Vol h1 = c.conv3(path, "head1.w", "head1.b", F / 2, one, ACT_NONE, nullptr, nullptr, nullptr);
    // dpt_head.py:79-84: interpolate -> head conv.  Knob conv_ups = 1 (off by default: measured slower, include/l4p_hip.h): where the
    // LDS-halo kernel's fused loader takes the shape (16-bit engines, time axis not resized, 128 output channels, whole 2 x 16 x 16
    // blocks: the full geometry) the up-sampled volume never exists
    Vol h2;
    const bool fuse = is16(c.dt) && knob(KNOB_CONV_UPS) && cfg->out_t == h1.t && (cfg->out_h != h1.h || cfg->out_w != h1.w) &&
                      cfg->last_dim == 128 && h1.c % 32 == 0 && cfg->out_t % 2 == 0 && cfg->out_h % 16 == 0 && cfg->out_w % 16 == 0 &&
                      (long long)c.B * cfg->out_t * cfg->out_h * cfg->out_w / 512 >= 192 &&
                      (long long)c.B * cfg->out_t * cfg->out_h * cfg->out_w * h1.c * 2 < (1ll << 32);
    if (fuse && !c.dry) {  // (the workspace is sized for the un-fused form: the knob may change between sizing and a forward)
        h2 = c.conv3(h1, "head2.w", "head2.b", cfg->last_dim, one, ACT_RELU, nullptr, nullptr, nullptr, cfg->out_h, cfg->out_w);
    } else {
        Vol h1u = c.resize(h1, cfg->out_t, cfg->out_h, cfg->out_w);
        h2 = c.conv3(h1u, "head2.w", "head2.b", cfg->last_dim, one, ACT_RELU, nullptr, nullptr, nullptr);
    }
    c.launch([&] {
        return launch_head_out(c.dt, h2.p, c.Wf("out.w"), c.Wf("out.b"), out, (long long)h2.t * h2.h * h2.w, c.B, cfg->last_dim,
                               cfg->out_ch, cfg->post_exp, c.st);
    });
    return c.rc;
}

}  // namespace

extern "C" {

size_t l4p_dpt_workspace_bytes(const l4p_engine* e, const l4p_dpt_cfg* cfg, int B) {
    if (!e || !cfg || B <= 0) return 0;
    Ctx c(e, B);
    const void* hooks[4] = {nullptr, nullptr, nullptr, nullptr};
    run(c, cfg, hooks, nullptr);
    return c.ws.bytes_needed();
}

int l4p_dpt_forward(l4p_engine* e, l4p_stream stream, const char* task, const l4p_dpt_cfg* cfg, const void* const* hooks, int B,
                    void* workspace, size_t ws_bytes, float* out) {
    if (!e || !task || !cfg || !hooks || !workspace || !out || B <= 0) {
        l4p_set_error("l4p_dpt_forward: bad arguments");
        return L4P_E_INVALID;
    }
    Ctx c(e, B, std::string("dpt.") + task + ".");
    c.on(stream, workspace, ws_bytes);
    return run(c, cfg, hooks, out);
}
}
