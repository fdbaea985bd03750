// The launch schedules: Builder (weight folding, tiling and upload, one Op per launch) and the three networks built with it (HRNet-W48 + head,
// YOLOv8 detect, OSNet-x0.25), and finalize(), which builds them and the step buffers of a handle.
#include "runtime.h"

namespace eagle {

// ------------------------------------------------------------------------------------------------------------
// Builder: shared by both networks
// ------------------------------------------------------------------------------------------------------------
struct Builder {
    EagleHandle* H;
    Net* net;
    int prec;
    double bn_eps;
    int N;
    const char* label_suffix = "";          // appended to the convolution labels of this network (" d": the detector, so that profiles can tell the networks apart)
    int cur_stream = 0;
    void set_stream(int k) { cur_stream = k; net->pool = k; }
    void fork_join(Op::Kind kind, int nbranch) { Op op; op.kind = kind; op.nbranch = nbranch; op.tag = kind == Op::FORK ? "fork" : "join"; net->ops.push_back(op); }

    int gran() const { return prec == EAGLE_PREC_F32 ? 4 : 8; }

    TView act(int h, int w, int c, bool f32 = false)
    {
        TView v; v.n = N; v.h = h; v.w = w; v.c = c; v.cs = c; v.off = 0;
        v.f32 = (f32 || prec == EAGLE_PREC_F32) ? 1 : prec_tensor_fmt(prec);
        v.p = net->get((size_t)N * h * w * c * v.esize());
        return v;
    }
    void release(const TView& v) { net->put(v.p); }

    const HostTensor& W(const std::string& name)
    {
        auto it = H->weights.find(name);
        if (it == H->weights.end()) fail(EAGLE_E_MISSING, "weight tensor '%s' was not loaded", name.c_str());
        return it->second;
    }

    // conv (+ folded BN when bn != ""), output into `out` if given (a slice of a concat buffer), else a new tensor.
    TView conv(const TView& x, const std::string& cname, const std::string& bn, int stride, int pre, const TView* r1,
               const TView* r2, int post, const TView* out = nullptr, bool out_f32 = false, ArgmaxPart* const* am_slot = nullptr)
    {
        std::vector<float> hwio, bias; int cin, cout, ks;
        fold(cname, bn, hwio, bias, cin, cout, ks);
        if (cin > x.c) fail(EAGLE_E_INVALID, "%s: input has %d channels, weight expects %d", cname.c_str(), x.c, cin);
        const int cout_pad = (cout + 15) / 16 * 16;
        bias.resize(cout_pad, 0.f);
        const int ho = (x.h + 2 * (ks / 2) - ks) / stride + 1, wo = (x.w + 2 * (ks / 2) - ks) / stride + 1;
        if (const char* dump = getenv("EAGLE_DUMP_LAYERS")) {
            if (FILE* f = fopen(dump, "a")) { fprintf(f, "%d,%d,%d,%d,%d,%d,%d\n", ks, stride, x.c, cout_pad, x.h, x.w, N); fclose(f); }
        }
        ConvLaunch L;
        L.cfg = conv_choose(prec, ks, stride, x.c, cout_pad, wo, pre == ACT_NONE && post <= ACT_RELU && !out_f32, r1 && r2);
        if (!conv_supported(prec, L.cfg))
            fail(EAGLE_E_NOKERNEL, "%s: no kernel instance (ks=%d s=%d kc=%d nt=%d)", cname.c_str(), ks, stride, L.cfg.kc, L.cfg.nt);
        const size_t ne = conv_weight_elems(prec, L.cfg);
        std::vector<char> tiled(ne * (prec == EAGLE_PREC_F32 ? 4 : 2));
        conv_tile_weights(prec, L.cfg, hwio.data(), cin, cout, tiled.data(), &L.descale);
        L.w = net->upload(tiled.data(), tiled.size());
        L.bias = (const float*)net->upload(bias.data(), bias.size() * 4);
        L.x = x;
        if (out) {
            L.y = *out;
            if (out->c != cout_pad || out->h != ho || out->w != wo) fail(EAGLE_E_INVALID, "%s: output slice mismatch", cname.c_str());
        } else {
            L.y = act(ho, wo, cout_pad, out_f32);
        }
        if (r1) L.r1 = *r1;
        if (r2) L.r2 = *r2;
        L.pre_act = pre; L.post_act = post; L.out_f32 = out_f32 ? 1 : 0;
        refuse_2gib(cname, "layer", {&L.x, &L.y, r1 ? &L.r1 : nullptr, r2 ? &L.r2 : nullptr});
        L.am_slot = am_slot;
        if (prec == EAGLE_PREC_F32S && !out_f32 && !am_slot) L.sat_slot = &H->cur_sat;
        if (am_slot) { H->hm_chunks = conv_tiles_per_frame(prec, L.cfg, ho, wo); H->fused_argmax = true; }
        L.flop = 2.0 * N * ho * wo * (double)cout * cin * ks * ks;
        const int pr = prec;
        char label[64];
        snprintf(label, sizeof(label), "conv %dx%d/%d %d->%d @%dx%d v%d%s", ks, ks, stride, cin, cout, ho, wo, L.cfg.variant, label_suffix);      // v: kernel form (conv.hip)
        // algorithmic HBM bytes of the launch: input once, output once, each residual once, weights once
        const double es = prec == EAGLE_PREC_F16 ? 2 : 4;
        emit_conv(label, L.flop, (double)N * x.h * x.w * cin * es + (double)N * ho * wo * cout * ((out_f32 || prec != EAGLE_PREC_F16) ? 4 : 2) * (am_slot ? 0 : 1) +
                                 (r1 ? (double)N * ho * wo * cout * es : 0) + (r2 ? (double)N * ho * wo * cout * es : 0) + (double)ks * ks * cin * cout * es,
                  [L, pr](hipStream_t s) { conv_launch(pr, L, s); });
        return L.y;
    }
    // weights of conv `cname` as [tap][cin][cout] and its bias, BatchNorm `bn` folded in: scale = gamma / sqrt(var + eps) (float64); w' = f32(f64(w) * scale); b' = f32(beta - mean * scale).
    // bn == "": the raw weights and the convolution's own bias, or zeros (a linear convolution without BatchNorm and bias: OSNet's LightConv3x3.conv1)
    void fold(const std::string& cname, const std::string& bn, std::vector<float>& hwio, std::vector<float>& bias, int& cin, int& cout, int& ks)
    {
        const HostTensor& w = W(cname + ".weight");
        if (w.shape.size() != 4) fail(EAGLE_E_INVALID, "%s.weight: expected 4-d", cname.c_str());
        cout = (int)w.shape[0]; cin = (int)w.shape[1]; ks = (int)w.shape[2];
        hwio.assign((size_t)ks * ks * cin * cout, 0.f); bias.assign(cout, 0.f);
        std::vector<double> scale(cout, 1.0);
        if (!bn.empty()) {
            const HostTensor &g = W(bn + ".weight"), &b = W(bn + ".bias"), &m = W(bn + ".running_mean"), &v = W(bn + ".running_var");
            for (int o = 0; o < cout; ++o) {
                scale[o] = (double)g.data[o] / std::sqrt((double)v.data[o] + bn_eps);
                bias[o] = (float)((double)b.data[o] - (double)m.data[o] * scale[o]);
            }
        } else if (H->weights.count(cname + ".bias")) {
            const HostTensor& b = W(cname + ".bias");
            for (int o = 0; o < cout; ++o) bias[o] = b.data[o];
        }
        for (int o = 0; o < cout; ++o)
            for (int i = 0; i < cin; ++i)
                for (int t = 0; t < ks * ks; ++t) {
                    const float wv = w.data[((size_t)o * cin + i) * ks * ks + t];
                    hwio[((size_t)t * cin + i) * cout + o] = bn.empty() ? wv : (float)((double)wv * scale[o]);
                }
    }
    // every convolution kernel addresses its tensors through raw buffer descriptors with 32-bit byte offsets: a tensor that reaches 2 GiB is
    // refused HERE (eagle_finalize_weights returns the error), not at the first launch in the middle of a pipeline or a hipGraph capture
    void refuse_2gib(const std::string& name, const char* what, std::initializer_list<const TView*> ts)
    {
        for (const TView* t : ts)
            if (t && (size_t)t->n * t->h * t->w * t->cs * t->esize() >= ((size_t)1 << 31))
                fail(EAGLE_E_INVALID, "%s: a %d x %d x %d x %d-channel tensor of this %s reaches 2 GiB at a device batch of %d frames (32-bit tensor offsets); use a smaller EagleConfig.batch",
                     name.c_str(), t->n, t->h, t->w, t->cs, what, N);
    }
    // names the launch (profiles key on the label) and appends it to the schedule of the stream being emitted for
    void emit_conv(const char* label, double flop, double bytes, std::function<void(hipStream_t)> run)
    {
        net->names.emplace_back(new std::string(label));
        Op op; op.kind = Op::CONV; op.flop = flop; op.bytes = bytes; op.tag = net->names.back()->c_str(); op.stream = cur_stream; op.run = std::move(run);
        net->ops.push_back(op);
    }
    // One launch for a whole Bottleneck (bneck.hip): relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + res), kh.py:101-137
    // ds_conv / ds_bn non-empty (block 0: Cin = 64): the 1 x 1 downsample branch of the shortcut is computed inside the launch (conv3 over K = 128 = [t2 | x], one weight
    // scale, bias b3 + bd) and `res` is not read
    TView bottleneck(const TView& x, const std::string& q, const TView& res, const std::string& ds_conv = "", const std::string& ds_bn = "")
    {
        BneckLaunch L;
        const bool dsf = !ds_conv.empty();
        std::vector<float> hw, bs; int ci, co, ks;
        std::vector<_Float16> img;
        double flop = 0;
        const char* cn[3] = {"conv1", "conv2", "conv3"}; const char* bnn[3] = {"bn1", "bn2", "bn3"};
        const int want_ks[3] = {1, 3, 1}, want_ci[3] = {x.c, 64, 64}, want_co[3] = {64, 64, 256};
        for (int k = 0; k < 3; ++k) {
            fold(q + cn[k], q + bnn[k], hw, bs, ci, co, ks);
            if (ks != want_ks[k] || ci != want_ci[k] || co != want_co[k]) fail(EAGLE_E_INVALID, "%s%s: not the Bottleneck shape of the fused kernel", q.c_str(), cn[k]);
            if (k == 2 && dsf) {                            // conv3's K dimension extended by the downsample branch: rows 0 .. 63 = W3 (over t2), rows 64 .. 127 = Wd (over x)
                std::vector<float> hwd, bd; int cid, cod, ksd;
                fold(ds_conv, ds_bn, hwd, bd, cid, cod, ksd);
                if (ksd != 1 || cid != 64 || cod != 256 || x.c != 64) fail(EAGLE_E_INVALID, "%s: not the 1x1 64->256 downsample of the fused kernel", ds_conv.c_str());
                hw.insert(hw.end(), hwd.begin(), hwd.end());
                for (int o = 0; o < 256; ++o) bs[o] = bs[o] + bd[o];
                ci = 128;
                flop += 2.0 * N * x.h * x.w * 256.0 * 64;
            }
            float ds = 1.f;
            bneck_tile_weights(hw.data(), ks * ks, ci, co, img, &ds);
            bneck_scale_bias(bs, ds);
            const void* dw = net->upload(img.data(), img.size() * 2);
            const float* db = (const float*)net->upload(bs.data(), bs.size() * 4);
            if (k == 0) { L.w1 = dw; L.b1 = db; L.ds1 = ds; } else if (k == 1) { L.w2 = dw; L.b2 = db; L.ds2 = ds; } else { L.w3 = dw; L.b3 = db; L.ds3 = ds; }
            flop += 2.0 * N * x.h * x.w * (double)co * (k == 2 ? 64 : ci) * ks * ks;
        }
        L.x = x; L.y = act(x.h, x.w, 256); L.res = dsf ? L.y : res; L.ds_fused = dsf;
        L.sat_slot = &H->cur_sat;
        refuse_2gib(q, "block", {&L.x, &L.y, &L.res});
        char label[64];
        snprintf(label, sizeof(label), "bneck %d->64->256%s @%dx%d%s", x.c, dsf ? "+ds" : "", x.h, x.w, label_suffix);
        emit_conv(label, flop, (double)N * x.h * x.w * 4.0 * (x.c + 256 + ((dsf || res.p == x.p) ? 0 : 256)) + 4.0 * (x.c * 64 + 9 * 64 * 64 + 64 * 256 + (dsf ? 64 * 256 : 0)),      // x once, y once (+ a separate residual tensor), weights once
                  [L](hipStream_t s) { bneck_launch(L, s); });
        return L.y;
    }
    // One launch from the frames to conv1's output (stem.hip): cv2.resize + A.Normalize + relu(bn1(conv1 3x3/2 3->64)).  x_in carries the shape only (no memory);
    // the frames and their number are read from the handle when the launch is enqueued (cur_src / cur_n)
    TView stem(const TView& x_in, const std::string& cname, const std::string& bn)
    {
        std::vector<float> hwio, bias; int cin, cout, ks;
        fold(cname, bn, hwio, bias, cin, cout, ks);
        if (!stem_supported(prec, ks, 2, cin, cout)) fail(EAGLE_E_NOKERNEL, "%s: not the 3x3/2 3->64 convolution of the fused stem", cname.c_str());
        StemLaunch L;
        std::vector<_Float16> img;
        stem_tile_weights(hwio.data(), img, &L.descale);
        L.w = net->upload(img.data(), img.size() * 2);
        L.bias = (const float*)net->upload(bias.data(), bias.size() * 4);
        L.sh = H->cfg.frame_h; L.sw = H->cfg.frame_w; L.dh = x_in.h; L.dw = x_in.w;
        L.y = act((x_in.h - 1) / 2 + 1, (x_in.w - 1) / 2 + 1, 64);
        L.sat_slot = &H->cur_sat;
        refuse_2gib(cname, "layer", {&L.y});
        const double flop = 2.0 * N * L.y.h * L.y.w * 64.0 * 27;
        char label[64];
        snprintf(label, sizeof(label), "conv stem 3x3/2 3->64 @%dx%d%s", L.y.h, L.y.w, label_suffix);
        EagleHandle* const Hh = H;
        // algorithmic HBM bytes: the frames once, the output once, weights once
        emit_conv(label, flop, (double)N * L.sh * L.sw * 3.0 + (double)N * L.y.h * L.y.w * 64 * 4.0 + 27.0 * 64 * 4,
                  [L, Hh](hipStream_t s) { StemLaunch l = L; l.bgr = Hh->cur_src; l.n = Hh->cur_n; stem_launch(l, s); });
        return L.y;
    }
    static double vbytes(const TView& v) { return (double)v.n * v.h * v.w * v.c * (v.f32 ? 4 : 2); }
    void other(std::function<void(hipStream_t)> fn, const char* tag, double bytes = 0)
    {
        Op op; op.kind = Op::OTHER; op.run = std::move(fn); op.tag = tag; op.stream = cur_stream; op.bytes = bytes;
        net->ops.push_back(op);
    }
};

// ------------------------------------------------------------------------------------------------------------
// HRNet-W48 + head (eagle/models/keypoint_hrnet.py:315-351, 444-481, 283-309, 553-562).  The fusion plan
// (which adds ride in which epilogue) is the one oracle/nets.py::_hr_stage mirrors.
// ------------------------------------------------------------------------------------------------------------
static const char* HRP = "unnormalized_model.0.";

static std::vector<TView> hr_stage(Builder& B, std::vector<TView> xs, int stage_idx, int n_modules, int nb, bool last_single)
{
    const int R = ACT_RELU;
    for (int m = 0; m < n_modules; ++m) {
        const std::string q = std::string(HRP) + "stage" + std::to_string(stage_idx) + "." + std::to_string(m) + ".";
        B.fork_join(Op::FORK, nb - 1);          // the branches of a module are independent until the fuse
        // emission order (= host launch order, and node order of a captured graph): block k of every branch before block k + 1 of any, the widest branch first —
        // a branch's first launch is then not queued behind the whole chains of the branches before it: one-frame call 6.74 -> 6.63 ms, four frames 8.62 -> 8.46
        // (profiles/r06ag_*; EAGLE_HR_INTERLEAVE=0: branch after branch)
        const bool interleave = !(getenv("EAGLE_HR_INTERLEAVE") && atoi(getenv("EAGLE_HR_INTERLEAVE")) == 0);
        for (int step = 0; step < 4 * nb; ++step) {
            const int k = interleave ? step / nb : step % 4, b = interleave ? nb - 1 - step % nb : step / 4;
            B.set_stream(b);
            TView x = xs[b];
            const std::string r = q + "branches." + std::to_string(b) + "." + std::to_string(k) + ".";
            TView o = B.conv(x, r + "conv1", r + "bn1", 1, 0, nullptr, nullptr, R);
            TView y = B.conv(o, r + "conv2", r + "bn2", 1, 0, &x, nullptr, R);
            B.release(o);
            B.release(x);
            xs[b] = y;
        }
        B.set_stream(0);
        B.fork_join(Op::JOIN, nb - 1);
        const int n_out = (last_single && m == n_modules - 1) ? 1 : nb;
        std::vector<TView> out;
        // (round 6) The fuse outputs are independent of each other: output i — its chain of stride-2 convolutions from the higher-resolution branches, its 1 x 1
        // convolutions of the lower ones, its fuse_sum — is emitted for stream i, so that with branch streams on (every batch since this round) the module's 19 fuse launches are
        // four parallel chains of at most 6 instead of one serial chain behind the join: 7.5 -> 6.66 ms per one-frame call, +1.6 .. 2.8 % at B = 50 (r06aj, r06ak).  The inputs
        // xs[] are only read; everything a chain allocates and releases stays in its own stream's pool.  Same launches, same arithmetic.  (Measured and not kept: also
        // moving the launches that need only ONE branch's output in front of the join, behind that branch — nothing, twice: profiles/r06ai_*.)
        if (n_out > 1) B.fork_join(Op::FORK, n_out - 1);
        for (int i = 0; i < n_out; ++i) {
            B.set_stream(n_out > 1 ? i : 0);
            TView y; bool have_y = false;
            for (int j = 0; j < i; ++j) {
                TView t = xs[j];
                for (int k = 0; k < i - j; ++k) {
                    const std::string r = q + "fuse_layers." + std::to_string(i) + "." + std::to_string(j) + "." + std::to_string(k) + ".";
                    const bool last = k == i - j - 1;
                    TView nt;
                    if (!last) {
                        nt = B.conv(t, r + "0", r + "1", 2, 0, nullptr, nullptr, R);
                    } else {
                        const TView* ident = (j == i - 1) ? &xs[i] : nullptr;
                        const bool relu_now = ident && i == nb - 1;
                        nt = B.conv(t, r + "0", r + "1", 2, 0, have_y ? &y : nullptr, ident, relu_now ? R : 0);
                    }
                    if (k > 0) B.release(t);
                    t = nt;
                }
                if (have_y) B.release(y);
                y = t; have_y = true;
            }
            if (i == 0) y = xs[0];
            FuseUp ups[3]; int nu = 0;
            for (int j = i + 1; j < nb; ++j) {
                const std::string r = q + "fuse_layers." + std::to_string(i) + "." + std::to_string(j) + ".";
                ups[nu++].z = B.conv(xs[j], r + "0", r + "1", 1, 0, nullptr, nullptr, 0);
            }
            if (nu) {
                TView o = B.act(y.h, y.w, y.c);
                const TView base = y; FuseUp u0 = ups[0], u1 = ups[1], u2 = ups[2]; const int n_up = nu;
                EagleHandle* const Hh = B.H;
                B.other([base, u0, u1, u2, n_up, o, Hh](hipStream_t s) { FuseUp u[3] = {u0, u1, u2}; fuse_sum_launch(base, u, n_up, 1, o, s, Hh->cur_sat); }, "fuse_sum",
                        Builder::vbytes(base) + Builder::vbytes(o) + (nu > 0 ? Builder::vbytes(ups[0].z) : 0) + (nu > 1 ? Builder::vbytes(ups[1].z) : 0) + (nu > 2 ? Builder::vbytes(ups[2].z) : 0));
                for (int k = 0; k < nu; ++k) B.release(ups[k].z);
                if (i != 0) B.release(y);
                y = o;
            }
            out.push_back(y);
        }
        B.set_stream(0);
        if (n_out > 1) B.fork_join(Op::JOIN, n_out - 1);
        // inputs of this module's fuse are dead now (xs[0] may be aliased by out[0] only when nb == 1, never here)
        for (int b = 0; b < nb; ++b) B.release(xs[b]);
        xs = out;
    }
    return xs;
}

static TView build_hrnet(Builder& B, const TView& x_in)
{
    const int R = ACT_RELU;
    const std::string P = HRP;
    TView x = B.H->stem_on ? B.stem(x_in, P + "conv1", P + "bn1") : B.conv(x_in, P + "conv1", P + "bn1", 2, 0, nullptr, nullptr, R);
    TView x2 = B.conv(x, P + "conv2", P + "bn2", 2, 0, nullptr, nullptr, R);
    B.release(x); x = x2;
    for (int b = 0; b < 4; ++b) {
        const std::string q = P + "layer1." + std::to_string(b) + ".";
        // round 6: the whole Bottleneck as one launch in the split family (EAGLE_BNECK_FUSED=0: the three launches of rounds 1-5); block 0's downsample branch inside it
        // (EAGLE_BNECK_DS=0: as its own launch, the residual read back)
        const char* fe = getenv("EAGLE_BNECK_FUSED");
        const char* de = getenv("EAGLE_BNECK_DS");
        const bool fused = B.prec == EAGLE_PREC_F32S && !(fe && atoi(fe) == 0) && bneck_supported(x, 64, 256);
        const bool dsf = fused && b == 0 && x.c == 64 && !(de && atoi(de) == 0);
        TView res = x;
        if (b == 0 && !dsf) res = B.conv(x, q + "downsample.0", q + "downsample.1", 1, 0, nullptr, nullptr, 0);
        if (fused) {
            TView y = dsf ? B.bottleneck(x, q, x, q + "downsample.0", q + "downsample.1") : B.bottleneck(x, q, res);
            if (b == 0 && !dsf) B.release(res);
            B.release(x);
            x = y;
            continue;
        }
        TView o1 = B.conv(x, q + "conv1", q + "bn1", 1, 0, nullptr, nullptr, R);
        TView o2 = B.conv(o1, q + "conv2", q + "bn2", 1, 0, nullptr, nullptr, R);
        TView y = B.conv(o2, q + "conv3", q + "bn3", 1, 0, &res, nullptr, R);
        B.release(o1); B.release(o2);
        if (b == 0) B.release(res);
        B.release(x);
        x = y;
    }
    std::vector<TView> ys(2);
    B.fork_join(Op::FORK, 1);                               // the two transition convolutions read the same tensor: side by side where branch streams are on
    B.set_stream(1);
    ys[1] = B.conv(x, P + "transition1.1.0.0", P + "transition1.1.0.1", 2, 0, nullptr, nullptr, R);
    B.set_stream(0);
    ys[0] = B.conv(x, P + "transition1.0.0", P + "transition1.0.1", 1, 0, nullptr, nullptr, R);
    B.fork_join(Op::JOIN, 1);
    B.release(x);
    ys = hr_stage(B, ys, 2, 1, 2, false);
    ys.push_back(B.conv(ys.back(), P + "transition2.2.0.0", P + "transition2.2.0.1", 2, 0, nullptr, nullptr, R));
    ys = hr_stage(B, ys, 3, 4, 3, false);
    ys.push_back(B.conv(ys.back(), P + "transition3.3.0.0", P + "transition3.3.0.1", 2, 0, nullptr, nullptr, R));
    ys = hr_stage(B, ys, 4, 3, 4, true);
    // fp16 family: sigmoid + per-tile maxima ride in the head convolution's epilogue (no logit tensor in HBM); the exact family
    // keeps the fp32 logits and heat_argmax_kernel
    ArgmaxPart* const* am = (prec_is_f16_kernels(B.prec) && !getenv("EAGLE_NO_FUSED_ARGMAX")) ? &B.H->cur_parts : nullptr;
    TView logits = B.conv(ys[0], "unnormalized_model.1", "", 1, 0, nullptr, nullptr, 0, nullptr, true, am);
    B.release(ys[0]);
    return logits;
}

// ------------------------------------------------------------------------------------------------------------
// YOLOv8 detect (ultralytics graph).  Concats are channel slices of one buffer: producers write
// straight into their slice, consumers read slices; nothing is copied except the nearest-x2 upsample.
// ------------------------------------------------------------------------------------------------------------
struct YoloDims { int c[5]; int n[4]; };
static YoloDims yolo_dims(int variant)
{
    static const double D[5] = {0.33, 0.33, 0.67, 1.0, 1.0}, Wd[5] = {0.25, 0.5, 0.75, 1.0, 1.25};
    static const int MC[5] = {1024, 1024, 768, 512, 512};
    YoloDims y;
    const int base[5] = {64, 128, 256, 512, 1024};
    for (int i = 0; i < 5; ++i) y.c[i] = (int)std::ceil(std::min(base[i], MC[variant]) * Wd[variant] / 8.0) * 8;
    const int rep[4] = {3, 6, 6, 3};
    for (int i = 0; i < 4; ++i) y.n[i] = std::max((int)std::nearbyint(rep[i] * D[variant]), 1);
    return y;
}

struct YoloBuilder {
    Builder& B;
    int S = ACT_SILU;
    TView cv(const TView& x, const std::string& name, int stride = 1, const TView* r1 = nullptr, const TView* out = nullptr)
    {
        return B.conv(x, name + ".conv", name + ".bn", stride, S, r1, nullptr, 0, out);
    }
    // C2f writing its result into `out` (or a fresh tensor)
    TView c2f(const TView& x, int idx, int cout, int n, bool shortcut, const TView* out = nullptr)
    {
        const std::string p = "model." + std::to_string(idx);
        const int c = cout / 2;
        TView cat = B.act(x.h, x.w, (2 + n) * c);
        TView first = cat.slice(0, 2 * c);
        cv(x, p + ".cv1", 1, nullptr, &first);
        for (int k = 0; k < n; ++k) {
            TView in = cat.slice((1 + k) * c, c);
            TView t = cv(in, p + ".m." + std::to_string(k) + ".cv1");
            TView o = cat.slice((2 + k) * c, c);
            cv(t, p + ".m." + std::to_string(k) + ".cv2", 1, shortcut ? &in : nullptr, &o);
            B.release(t);
        }
        TView y = cv(cat, p + ".cv2", 1, nullptr, out);
        B.release(cat);
        return y;
    }
};

// mixed (EAGLE_DET_PREC_MIXED; VERDICT r5 task 7): the trunk in the split family, the LAST C2f of every level (model.15 / 18 / 21), the two stride-2 convolutions between them
// (model.16 / 19) and Detect (model.22) in the exact fp32 family; the seam is an exact conversion of the three concat buffers (split_to_f32_launch).
static void build_yolo(Builder& B, const TView& x_in, int variant, DetLevel lv[3], int nc, bool mixed = false)
{
    YoloBuilder Y{B};
    const YoloDims d = yolo_dims(variant);
    const int c1 = d.c[0], c2 = d.c[1], c3 = d.c[2], c4 = d.c[3], c5 = d.c[4];
    TView x0 = Y.cv(x_in, "model.0", 2);
    TView x1 = Y.cv(x0, "model.1", 2); B.release(x0);
    TView x2 = Y.c2f(x1, 2, c2, d.n[0], true); B.release(x1);
    TView x3 = Y.cv(x2, "model.3", 2); B.release(x2);
    const int h3 = x3.h, w3 = x3.w;                                   // stride 8
    const int h4 = (h3 - 1) / 2 + 1, w4 = (w3 - 1) / 2 + 1, h5 = (h4 - 1) / 2 + 1, w5 = (w4 - 1) / 2 + 1;
    // concat buffers of the head, allocated up-front so the backbone can write P3/P4/P5 into their slices
    TView cat15 = B.act(h3, w3, c4 + c3);      // [up(h12) | p3]
    TView cat12 = B.act(h4, w4, c5 + c4);      // [up(p5)  | p4]
    TView cat18 = B.act(h4, w4, c3 + c4);      // [conv16  | h12]
    TView cat21 = B.act(h5, w5, c4 + c5);      // [conv19  | p5]
    TView p3 = cat15.slice(c4, c3), p4 = cat12.slice(c5, c4), p5 = cat21.slice(c4, c5), h12 = cat18.slice(c3, c4);
    Y.c2f(x3, 4, c3, d.n[1], true, &p3); B.release(x3);
    TView x5 = Y.cv(p3, "model.5", 2);
    Y.c2f(x5, 6, c4, d.n[2], true, &p4); B.release(x5);
    TView x7 = Y.cv(p4, "model.7", 2);
    TView x8 = Y.c2f(x7, 8, c5, d.n[3], true); B.release(x7);
    {   // SPPF
        const int ch = c5 / 2;
        TView cat = B.act(h5, w5, 4 * ch);
        TView s0 = cat.slice(0, ch), s1 = cat.slice(ch, ch), s2 = cat.slice(2 * ch, ch), s3 = cat.slice(3 * ch, ch);
        Y.cv(x8, "model.9.cv1", 1, nullptr, &s0); B.release(x8);
        B.other([s0, s1](hipStream_t s) { maxpool5_launch(s0, s1, s); }, "maxpool5", 2 * Builder::vbytes(s0));
        B.other([s1, s2](hipStream_t s) { maxpool5_launch(s1, s2, s); }, "maxpool5", 2 * Builder::vbytes(s0));
        B.other([s2, s3](hipStream_t s) { maxpool5_launch(s2, s3, s); }, "maxpool5", 2 * Builder::vbytes(s0));
        Y.cv(cat, "model.9.cv2", 1, nullptr, &p5);
        B.release(cat);
    }
    {
        TView u = cat12.slice(0, c5);
        B.other([p5, u](hipStream_t s) { upsample2_launch(p5, u, s); }, "upsample2", Builder::vbytes(p5) + Builder::vbytes(u));
        Y.c2f(cat12, 12, c4, d.n[0], false, &h12);
    }
    TView h15, h18, h21;
    {
        TView u = cat15.slice(0, c4);
        B.other([h12, u](hipStream_t s) { upsample2_launch(h12, u, s); }, "upsample2", Builder::vbytes(h12) + Builder::vbytes(u));
    }
    if (!mixed) {
        h15 = Y.c2f(cat15, 15, c3, d.n[0], false);
        {
            TView o = cat18.slice(0, c3);
            Y.cv(h15, "model.16", 2, nullptr, &o);
        }
        h18 = Y.c2f(cat18, 18, c4, d.n[0], false);
        {
            TView o = cat21.slice(0, c4);
            Y.cv(h18, "model.19", 2, nullptr, &o);
        }
        h21 = Y.c2f(cat21, 21, c5, d.n[0], false);
    } else {
        B.prec = EAGLE_PREC_F32;                           // every tensor allocated and every convolution built from here on: the exact family
        auto to_f32 = [&B](const TView& x, const TView& y) {
            B.other([x, y](hipStream_t s) { split_to_f32_launch(x, y, s); }, "split_to_f32", Builder::vbytes(x) + Builder::vbytes(y));
        };
        TView cat15f = B.act(h3, w3, c4 + c3), cat18f = B.act(h4, w4, c3 + c4), cat21f = B.act(h5, w5, c4 + c5);
        to_f32(cat15, cat15f);
        h15 = Y.c2f(cat15f, 15, c3, d.n[0], false);
        {
            TView o = cat18f.slice(0, c3);
            Y.cv(h15, "model.16", 2, nullptr, &o);
            to_f32(h12, cat18f.slice(c3, c4));
        }
        h18 = Y.c2f(cat18f, 18, c4, d.n[0], false);
        {
            TView o = cat21f.slice(0, c4);
            Y.cv(h18, "model.19", 2, nullptr, &o);
            to_f32(p5, cat21f.slice(c4, c5));
        }
        h21 = Y.c2f(cat21f, 21, c5, d.n[0], false);
    }
    const TView feats[3] = {h15, h18, h21};
    const float strides[3] = {8.f, 16.f, 32.f};
    int a0 = 0;
    for (int l = 0; l < 3; ++l) {
        const std::string pb = "model.22.cv2." + std::to_string(l), pc = "model.22.cv3." + std::to_string(l);
        TView b0 = Y.cv(feats[l], pb + ".0");
        TView b1 = Y.cv(b0, pb + ".1"); B.release(b0);
        TView box = B.conv(b1, pb + ".2", "", 1, 0, nullptr, nullptr, 0, nullptr, true); B.release(b1);
        TView k0 = Y.cv(feats[l], pc + ".0");
        TView k1 = Y.cv(k0, pc + ".1"); B.release(k0);
        TView cls = B.conv(k1, pc + ".2", "", 1, 0, nullptr, nullptr, 0, nullptr, true); B.release(k1);
        lv[l].box = box; lv[l].cls = cls; lv[l].gh = box.h; lv[l].gw = box.w; lv[l].stride = strides[l]; lv[l].a0 = a0;
        a0 += box.h * box.w;
    }
    (void)c1; (void)nc;
}

// ------------------------------------------------------------------------------------------------------------
// OSNet-x0.25 (appearance embeddings of the tracker; architecture table in eagle_amd/osnet.py, kernels in reid.hip).  The 1 x 1
// convolutions are ordinary Builder convolutions in the exact fp32 family; everything else is a reid_* launch.
// ------------------------------------------------------------------------------------------------------------
static const char* RP = "reid.";

struct ReidFold { std::vector<float> scale, shift; };
static ReidFold reid_bn(Builder& B, const std::string& bn, int c)
{
    const HostTensor &g = B.W(bn + ".weight"), &b = B.W(bn + ".bias"), &m = B.W(bn + ".running_mean"), &v = B.W(bn + ".running_var");
    ReidFold f; f.scale.resize(c); f.shift.resize(c);
    for (int o = 0; o < c; ++o) {
        const double sc = (double)g.data[o] / std::sqrt((double)v.data[o] + 1e-5);
        f.scale[o] = (float)sc; f.shift[o] = (float)((double)b.data[o] - (double)m.data[o] * sc);
    }
    return f;
}

static TView reid_light(Builder& B, const TView& x, const std::string& lc, int mid)
{
    // LightConv3x3: 1x1 linear convolution -> depthwise 3x3 -> BatchNorm -> ReLU
    TView t = B.conv(x, lc + ".conv1", "", 1, 0, nullptr, nullptr, 0);
    const HostTensor& w = B.W(lc + ".conv2.weight");                       // [mid, 1, 3, 3]
    const ReidFold f = reid_bn(B, lc + ".bn", mid);
    const int C = t.c;
    std::vector<float> wk((size_t)9 * C, 0.f), bk(C, 0.f);
    for (int c = 0; c < mid; ++c) {
        for (int k = 0; k < 9; ++k) wk[(size_t)k * C + c] = (float)((double)w.data[(size_t)c * 9 + k] * (double)f.scale[c]);
        bk[c] = f.shift[c];
    }
    const float* dw = (const float*)B.net->upload(wk.data(), wk.size() * 4);
    const float* db = (const float*)B.net->upload(bk.data(), bk.size() * 4);
    TView y = B.act(t.h, t.w, C);
    const int n = B.N;
    B.other([t, dw, db, y, n](hipStream_t s) { reid_dw3_launch(t, dw, db, y, n, s); }, "reid dw3x3", 2 * Builder::vbytes(y));
    B.release(t);
    return y;
}

static TView reid_osblock(Builder& B, const TView& x, const std::string& b, int cin, int cout)
{
    const int mid = cout / 4, R = ACT_RELU;
    TView x1 = B.conv(x, b + ".conv1.conv", b + ".conv1.bn", 1, 0, nullptr, nullptr, R);
    TView st[4];
    st[0] = reid_light(B, x1, b + ".conv2a", mid);
    const char* names[3] = {"b", "c", "d"};
    for (int k = 0; k < 3; ++k) {
        TView y = x1;
        for (int d = 0; d < k + 2; ++d) {
            TView nx = reid_light(B, y, b + ".conv2" + names[k] + "." + std::to_string(d), mid);
            if (d > 0) B.release(y);
            y = nx;
        }
        st[k + 1] = y;
    }
    B.release(x1);
    // the shared ChannelGate and the four-stream sum
    const HostTensor &w1 = B.W(b + ".gate.fc1.weight"), &b1 = B.W(b + ".gate.fc1.bias"), &w2 = B.W(b + ".gate.fc2.weight"), &b2 = B.W(b + ".gate.fc2.bias");
    const int r = (int)w1.shape[0];
    const float* d1 = (const float*)B.net->upload(w1.data.data(), w1.data.size() * 4);
    const float* e1 = (const float*)B.net->upload(b1.data.data(), b1.data.size() * 4);
    const float* d2 = (const float*)B.net->upload(w2.data.data(), w2.data.size() * 4);
    const float* e2 = (const float*)B.net->upload(b2.data.data(), b2.data.size() * 4);
    const int C = st[0].c, n = B.N;
    float* g = (float*)B.net->get((size_t)n * 4 * C * 4);
    TView x2 = B.act(st[0].h, st[0].w, C);
    const TView s0 = st[0], s1 = st[1], s2 = st[2], s3 = st[3];
    B.other([s0, s1, s2, s3, d1, e1, d2, e2, mid, r, g, x2, n](hipStream_t s) { const TView ss[4] = {s0, s1, s2, s3}; reid_gate_launch(ss, d1, e1, d2, e2, mid, r, g, x2, n, s); },
            "reid gate", 5 * Builder::vbytes(x2));
    for (auto& t : st) B.release(t);
    TView ident = x;
    if (cin != cout) ident = B.conv(x, b + ".downsample.conv", b + ".downsample.bn", 1, 0, nullptr, nullptr, 0);
    TView y = B.conv(x2, b + ".conv3.conv", b + ".conv3.bn", 1, 0, &ident, nullptr, R);       // relu(conv3(x2) + identity): the residual add is commutative
    B.release(x2);
    if (cin != cout) B.release(ident);
    return y;
}

static void build_reid(Builder& B, EagleHandle* h)
{
    const std::string P = RP;
    const int n = B.N;
    h->reid_in = B.act(256, 128, 4);
    // stem: 7 x 7 / 2 convolution + BatchNorm + ReLU (weights [7][7][3][16] with the BN scale folded in), 3 x 3 / 2 max-pool
    const HostTensor& w1 = B.W(P + "conv1.conv.weight");                    // [16, 3, 7, 7]
    const ReidFold f1 = reid_bn(B, P + "conv1.bn", 16);
    std::vector<float> wk(7 * 7 * 3 * 16), bk(16);
    for (int o = 0; o < 16; ++o) {
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 49; ++k) wk[(size_t)(k * 3 + c) * 16 + o] = (float)((double)w1.data[((size_t)o * 3 + c) * 49 + k] * (double)f1.scale[o]);
        bk[o] = f1.shift[o];
    }
    const float* dw = (const float*)B.net->upload(wk.data(), wk.size() * 4);
    const float* db = (const float*)B.net->upload(bk.data(), bk.size() * 4);
    TView c1 = B.act(128, 64, 16);
    const TView in = h->reid_in;
    B.other([in, dw, db, c1, n](hipStream_t s) { reid_conv7_launch(in, dw, db, c1, n, s); }, "reid conv7x7", Builder::vbytes(in) + Builder::vbytes(c1));
    TView x = B.act(64, 32, 16);
    B.other([c1, x, n](hipStream_t s) { reid_maxpool3s2_launch(c1, x, n, s); }, "reid maxpool", Builder::vbytes(c1) + Builder::vbytes(x));
    B.release(c1);
    static const int CH[4] = {16, 64, 96, 128};
    const char* stage[3] = {"conv2", "conv3", "conv4"};
    for (int sI = 0; sI < 3; ++sI) {
        const int cin = CH[sI], cout = CH[sI + 1];
        const std::string sp = P + stage[sI];
        TView y = reid_osblock(B, x, sp + ".0", cin, cout); B.release(x); x = y;
        y = reid_osblock(B, x, sp + ".1", cout, cout); B.release(x); x = y;
        if (sI < 2) {                                       // transition: Conv1x1 + BN + ReLU, AvgPool2d(2, 2)
            TView t = B.conv(x, sp + ".2.0.conv", sp + ".2.0.bn", 1, 0, nullptr, nullptr, ACT_RELU); B.release(x);
            TView p = B.act(t.h / 2, t.w / 2, t.c);
            B.other([t, p, n](hipStream_t s) { reid_avgpool2_launch(t, p, n, s); }, "reid avgpool", Builder::vbytes(t) + Builder::vbytes(p));
            B.release(t);
            x = p;
        }
    }
    TView c5 = B.conv(x, P + "conv5.conv", P + "conv5.bn", 1, 0, nullptr, nullptr, ACT_RELU); B.release(x);
    // head: global average -> Linear(128, 512) + bias -> BatchNorm1d -> ReLU, the BN folded into the linear layer
    const HostTensor &fw = B.W(P + "fc.0.weight"), &fb = B.W(P + "fc.0.bias");
    const ReidFold ff = reid_bn(B, P + "fc.1", EAGLE_REID_DIM);
    std::vector<float> hw((size_t)EAGLE_REID_DIM * c5.c, 0.f), hb(EAGLE_REID_DIM);
    for (int o = 0; o < EAGLE_REID_DIM; ++o) {
        for (int c = 0; c < 128; ++c) hw[(size_t)o * c5.c + c] = (float)((double)fw.data[(size_t)o * 128 + c] * (double)ff.scale[o]);
        hb[o] = (float)((double)fb.data[o] * (double)ff.scale[o] + (double)ff.shift[o]);
    }
    const float* dhw = (const float*)B.net->upload(hw.data(), hw.size() * 4);
    const float* dhb = (const float*)B.net->upload(hb.data(), hb.size() * 4);
    h->reid_feats = (float*)B.net->get((size_t)n * EAGLE_REID_DIM * 4);
    float* feats = h->reid_feats;
    B.other([c5, dhw, dhb, feats, n](hipStream_t s) { reid_head_launch(c5, dhw, dhb, feats, EAGLE_REID_DIM, n, s); }, "reid head", Builder::vbytes(c5));
    h->reid_crops = (EagleCrop*)B.net->get(sizeof(EagleCrop) * (size_t)n);
    HIP_CHECK(hipHostMalloc((void**)&h->reid_crops_h, sizeof(EagleCrop) * (size_t)n, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void**)&h->reid_feats_h, sizeof(float) * EAGLE_REID_DIM * (size_t)n, hipHostMallocDefault));
}

void finalize(EagleHandle* h)
{
    const EagleConfig& c = h->cfg;
    const int B = c.batch;
    h->prec = c.precision;
    const bool det_mixed = c.det_precision == EAGLE_DET_PREC_MIXED;
    h->det_prec = det_mixed ? EAGLE_PREC_F32S : c.det_precision ? c.det_precision - 1 : c.precision;
    h->hr.reset(new Net); h->yo.reset(new Net); h->misc.reset(new Net);
    const int cin_pad = h->prec == EAGLE_PREC_F32 ? 4 : 8, det_cin_pad = h->det_prec == EAGLE_PREC_F32 ? 4 : 8;
    h->lb = letterbox_geometry(c.frame_h, c.frame_w, c.det_imgsz, c.letterbox);
    // inputs (written by the preprocess kernel)
    Builder Bh{h, h->hr.get(), h->prec, 1e-5, B};
    Builder By{h, h->yo.get(), h->det_prec, 1e-3, B};
    By.label_suffix = " d";
    // the split family's HRNet starts from the frames themselves (stem.hip): its input tensor is a shape without memory
    const HostTensor& w1 = Bh.W(std::string(HRP) + "conv1.weight");      // [cout, cin, ks, ks]
    h->stem_on = w1.shape.size() == 4 && stem_supported(h->prec, (int)w1.shape[2], 2, (int)w1.shape[1], (int)w1.shape[0]);
    if (h->stem_on) { TView v; v.n = B; v.h = 540; v.w = 960; v.c = v.cs = cin_pad; v.f32 = prec_tensor_fmt(h->prec); h->kp_in = v; }
    else h->kp_in = Bh.act(540, 960, cin_pad);
    h->det_in = By.act(h->lb.out_h, h->lb.out_w, det_cin_pad);
    h->logits = build_hrnet(Bh, h->kp_in);
    build_yolo(By, h->det_in, c.det_variant, h->levels, 5, det_mixed);
    if (h->weights.count(std::string(RP) + "conv1.conv.weight")) {          // appearance embeddings for the tracker: only when the caller loaded an OSNet
        h->reid.reset(new Net);
        Builder Br{h, h->reid.get(), EAGLE_PREC_F32, 1e-5, REID_NB};
        build_reid(Br, h);
    }
    // scratch
    Net* m = h->misc.get();
    for (auto& sb : h->sb) {
        sb.d_frames = (uint8_t*)m->get((size_t)B * c.frame_h * c.frame_w * 3);
        sb.parts = (ArgmaxPart*)m->get(sizeof(ArgmaxPart) * (size_t)B * h->hm_chunks * 64);
        const size_t sat_pad = sat_pad_bytes(B);
        sb.d_sat = (unsigned*)m->get(sat_pad + sizeof(EagleFrameResult) * (size_t)B);
        sb.d_out = (EagleFrameResult*)((char*)sb.d_sat + sat_pad);
        HIP_CHECK(hipHostMalloc((void**)&sb.h_sat, sat_pad + sizeof(EagleFrameResult) * (size_t)B, hipHostMallocDefault));
        sb.h_out = (EagleFrameResult*)((char*)sb.h_sat + sat_pad);
        HIP_CHECK(hipEventCreateWithFlags(&sb.ev_compute, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&sb.ev_done, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&sb.ev_copy, hipEventDisableTiming));
    }
    h->clip_sat = (unsigned*)m->get(sat_pad_bytes(B));
    HIP_CHECK(hipHostMalloc((void**)&h->clip_sat_h, sat_pad_bytes(B), hipHostMallocDefault));
    int A = 0;
    for (int l = 0; l < 3; ++l) A += h->levels[l].gh * h->levels[l].gw;
    h->ds.A = A;
    h->ds.boxes = (float*)m->get(sizeof(float) * 4 * (size_t)B * A);
    h->ds.conf = (float*)m->get(sizeof(float) * (size_t)B * A);
    h->ds.cls = (int*)m->get(sizeof(int) * (size_t)B * A);
    h->ds.keys = (unsigned long long*)m->get(sizeof(unsigned long long) * (size_t)B * A);
    h->ds.count = (int*)m->get(sizeof(int) * (size_t)B);
    PostParams& pp = h->pp;
    pp.frame_h = c.frame_h; pp.frame_w = c.frame_w; pp.in_h = h->lb.out_h; pp.in_w = h->lb.out_w;
    pp.hm_h = h->logits.h; pp.hm_w = h->logits.w; pp.hm_chunks = h->hm_chunks;
    pp.keypoint_conf = c.keypoint_conf; pp.detector_conf = c.detector_conf; pp.nms_iou = c.nms_iou;
    pp.ransac_thresh = c.ransac_thresh; pp.ransac_max_iters = c.ransac_max_iters; pp.lm_iters = c.lm_iters;
    h->n_conv = 0; h->conv_flop_step = 0; h->n_launch = 6;
    for (Net* n : {h->hr.get(), h->yo.get()})
        for (Op& op : n->ops) { ++h->n_launch; if (op.kind == Op::CONV) { ++h->n_conv; h->conv_flop_step += op.flop; } }
    h->conv_ev.resize((size_t)h->n_conv * 2);
    for (auto& e : h->conv_ev) HIP_CHECK(hipEventCreate(&e));
    h->weights.clear();      // host copies are no longer needed
    // Net::get zeroes on the null stream, which the handle's non-blocking streams do not wait for: while another handle keeps the GPU busy a zeroing of the
    // scratch above (staged frames, NMS keys, records) could still be queued when the first step writes them
    HIP_CHECK(hipStreamSynchronize(nullptr));
    h->finalized = true;
}

}  // namespace eagle
