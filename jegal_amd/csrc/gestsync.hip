// libjegal_hip: GestSync -- finalize, const chain, conv stacks, transformer (fused plan; unfused plan per arithmetic), clip and window paths.  Host code only.
#include "engine.h"

namespace engine {

// conv1 .. conv5 of the video CNN; conv2 .. conv5 take their taps in parity-class order, as packed (make_conv(..., reorder = true))
static void gs_conv_geoms(ConvGeom g[5]) {
    g[0] = geom(FH, FW, 16, 7, 7, 3, 3, 0, 0);             // 88 x 158
    g[1] = geom(43, 78, 64, 5, 5, 2, 2, 0, 0, true);       // 20 x 37
    g[2] = geom(20, 37, 128, 3, 3, 2, 2, 1, 1, true);      // 10 x 19
    g[3] = geom(10, 19, 256, 3, 3, 1, 2, 1, 1, true);      // 10 x 10
    g[4] = geom(10, 10, 256, 3, 3, 1, 1, 1, 1, true);      // 10 x 10
}

// Const chain (ConvGeom::rowskip): conv2 .. conv5 of an all-constant pooled image -- relu(bias1) in every pixel, which is
// what conv1 + max-pool produce wherever the frames are blanked.  Computed once per weight load with the run-time kernels
// (same MFMA sequence per output element, so the rows are bit-identical to what the layers would compute per position);
// 4 copies per layer so that every launch has the 256 rows the LDS-DMA kernel needs.
static int gs_build_const_chain(jg_handle* h) {
    GestSyncModel& gs = h->gs;
    gs.c2C = gs.c3C = gs.c4C = gs.c5C = nullptr;
    // (option gemm_glds is the policy here -- the chain is built before any launch shape is known; which launches then reach the LDS-DMA
    // conv kernel is plan_gemm's answer, gs_conv_stack)
    if (!h->opts.gemm_glds || h->bf16) return JG_OK;      // the chain starts from conv1_direct's constant (fp16 build only)
    constexpr int NC = 4;
    f16 *zc, *poolC, *c2C, *c3C, *c4C, *c5C;
    RET(walloc(h, gs.m, (size_t)64, &zc));
    RET(walloc(h, gs.m, (size_t)NC * 43 * 78 * 64, &poolC));
    RET(walloc(h, gs.m, (size_t)NC * 20 * 37 * 128, &c2C));
    RET(walloc(h, gs.m, (size_t)NC * 10 * 19 * 256, &c3C));
    RET(walloc(h, gs.m, (size_t)NC * 10 * 10 * 256, &c4C));
    RET(walloc(h, gs.m, (size_t)NC * 10 * 10 * 256, &c5C));
    HIPCHK(h, launch_conv1_zconst(gs.c1_direct, 1.0f / 255.0f, zc, h->stream));
    HIPCHK(h, launch_broadcast_channels(zc, 64, poolC, (long)NC * 43 * 78, h->stream));
    ConvGeom g[5];
    gs_conv_geoms(g);
    Epi e;
    e.relu = 1;
    e.out16 = c2C; RET(gemm(h, JG_ST_CONV, poolC, 0, NC * 20 * 37, gs.c2, e, &g[1]));
    e.out16 = c3C; RET(gemm(h, JG_ST_CONV, c2C, 0, NC * 10 * 19, gs.c3, e, &g[2]));
    e.out16 = c4C; RET(gemm(h, JG_ST_CONV, c3C, 0, NC * 10 * 10, gs.c4, e, &g[3]));
    e.out16 = c5C; RET(gemm(h, JG_ST_CONV, c4C, 0, NC * 10 * 10, gs.c5, e, &g[4]));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    gs.c2C = c2C; gs.c3C = c3C; gs.c4C = c4C; gs.c5C = c5C;
    return JG_OK;
}

int finalize_gestsync(jg_handle* h) {
    drop_model(h, h->gs);
    GestSyncModel& gs = h->gs;
    Model& m = gs.m;
    PackedLayer c1;
    RET(pack_conv(h, m.id, "net_vid.conv1", "net_vid.bn1", {64, 3, 5, 7, 7, 16, 0, 0, 1, 1, false}, LK_CONV, &c1));
    static_assert(CONV1_PANEL_O == 64 && CONV1_PANEL_K == 7 * 7 * 16, "the direct kernel's panel is conv1 as packed here");
    std::vector<uint16_t> c1_direct;          // conv1_direct_kernel's slot-major panel (fp16 build only), from the host result
    if (!h->bf16) c1_direct = conv1_direct_panel(c1.hi.data(), c1.bias.data());
    RET(upload_layer(h, m, std::move(c1), &gs.c1));
    // conv2..conv5: taps grouped by stride parity class (ConvGeom::taps); gs_conv_geoms builds the same geometry
    RET(make_conv(h, m, "net_vid.conv2", "net_vid.bn2", 128, 64, 1, 5, 5, 64, 0, &gs.c2, 2, 2, true));
    RET(make_conv(h, m, "net_vid.conv3", "net_vid.bn3", 256, 128, 1, 3, 3, 128, 0, &gs.c3, 2, 2, true));
    RET(make_conv(h, m, "net_vid.conv4", "net_vid.bn4", 256, 256, 1, 3, 3, 256, 0, &gs.c4, 1, 2, true));
    RET(make_conv(h, m, "net_vid.conv5", "net_vid.bn5", 256, 256, 1, 3, 3, 256, 0, &gs.c5, 1, 1, true));
    RET(make_conv(h, m, "net_vid.fc6", "net_vid.bn6", 512, 256, 1, 4, 4, 256, 0, &gs.fc6));
    RET(upload(h, m, std::vector<float>(64, 1.0f / 255.0f), &gs.c1_scale255));
    if (!h->bf16) RET(upload(h, m, c1_direct, &gs.c1_direct));
    RET(make_linear(h, m, "ff_vid.0.weight", "ff_vid.0.bias", 512, 512, &gs.ff0));
    RET(make_linear(h, m, "ff_vid.2.weight", "ff_vid.2.bias", 1024, 512, &gs.ff2));
    const HostTensor* pe;
    RET(need(h, "pos_encoder.pe", 50 * 512, &pe));
    RET(upload(h, m, pe->v, &gs.pe));
    for (int l = 0; l < 6; ++l) {
        const std::string p = "transformer_encoder.layers." + std::to_string(l);
        EncLayer* L = &gs.layers[l];
        RET(make_linear(h, m, p + ".self_attn.in_proj_weight", p + ".self_attn.in_proj_bias", 1536, 512, &L->qkv));
        RET(make_linear(h, m, p + ".self_attn.out_proj.weight", p + ".self_attn.out_proj.bias", 512, 512, &L->out));
        RET(make_linear(h, m, p + ".linear1.weight", p + ".linear1.bias", 2048, 512, &L->ff1));
        RET(make_linear(h, m, p + ".linear2.weight", p + ".linear2.bias", 512, 2048, &L->ff2));
        RET(make_ln(h, m, p + ".norm1.weight", p + ".norm1.bias", 512, &L->n1));
        RET(make_ln(h, m, p + ".norm2.weight", p + ".norm2.bias", 512, &L->n2));
    }
    m.ready = true;
    return gs_build_const_chain(h);
}

// conv1 + max-pool straight from u8 frames: zero-band scan (stage "conv1_aux"), the fused kernel (stage "conv1": the
// path's dominant kernel, timed alone), strip-seam fix-up (stage "conv1_aux")
// fill_all = false: the caller's conv2 honours the row skip the scan leaves in zscr, so the pooled rows it never reads stay unwritten
static int conv1_from_frames(jg_handle* h, const uint8_t* src, int nclip, int T, int pad, f16* pooled, f16* edge, unsigned* zscr, bool fill_all) {
    const bool scan = h->opts.conv1_zero_skip;
    const f16* wd = h->gs.c1_direct;
    if (debug_sync()) {
        const long NFd = (long)nclip * (T + 2 * pad - 4);
        std::fprintf(stderr, "[jg] conv1: src %p..%p pooled %p..%p edge %p..%p zscr %p..%p fill_all %d\n", (const void*)src,
                     (const void*)(src + (size_t)nclip * T * FH * FW * 3), (void*)pooled, (void*)(pooled + (size_t)NFd * 43 * 78 * 64), (void*)edge,
                     (void*)(edge + conv1_edge_elems(NFd)), (void*)zscr, (void*)(zscr + conv1_zmask_elems(nclip, T)), (int)fill_all);
    }
    if (scan) RET(timed(h, JG_ST_CONV1_AUX, [&] { return launch_conv1_scan(src, nclip, T, pad, wd, 1.0f / 255.0f, zscr, h->stream); }));
    RET(timed(h, JG_ST_CONV1, [&] { return launch_conv1_direct(src, nclip, T, pad, wd, 1.0f / 255.0f, pooled, edge,
                                                               scan ? zscr : nullptr, fill_all, h->opts, h->stream); }));
    return timed(h, JG_ST_CONV1_AUX, [&] { return launch_conv1_edge_fix(pooled, edge, (long)nclip * (T + 2 * pad - 4), h->stream); });
}

// conv1 + max-pool of `nclip` temporal volumes -> pooled (nclip*P, 43, 78, 64) fp16, P = T + 2*pad - 4; *zscr: the zero-band scan of the
// direct kernel (conv1_from_frames), nullptr otherwise
int gs_conv1_stage(jg_handle* h, const void* src, int src_u8, long sb, long st, long sh, long sw, long sc, int nclip, int T, int pad,
                   f16* pooled, bool fill_all, unsigned** zscr) {
    const long NF = (long)nclip * (T + 2 * pad - 4);
    // (the direct kernel feeds u8 pixels to the MFMA as fp16 subnormals: fp16 build only; JG_PREC_BF16 stacks the frames and runs
    // conv1 as an implicit GEMM)
    const bool direct = src_u8 && sc == 1 && sw == 3 && sh == (long)FW * 3 && st == (long)FH * FW * 3 && sb == (long)T * st && h->conv1_direct && !h->bf16;
    *zscr = nullptr;
    if (direct) {
        // u8 HWC video: conv1 + max-pool straight from the frames; neither the temporal stack nor the
        // pre-pool tensor exists in HBM
        f16* edge;
        RET(wsalloc(h, conv1_edge_elems(NF), &edge));
        RET(wsalloc(h, conv1_zmask_elems(nclip, T), zscr));
        return conv1_from_frames(h, static_cast<const uint8_t*>(src), nclip, T, pad, pooled, edge, *zscr, fill_all);
    }
    f16 *o1, *S;
    RET(wsalloc(h, (size_t)NF * 88 * 158 * 64, &o1));
    RET(wsalloc(h, (size_t)NF * FH * FW * 16, &S));
    ConvGeom g[5];
    gs_conv_geoms(g);
    RET(timed(h, JG_ST_STACK, [&] { return LAUNCH(h, launch_stack_frames, src, src_u8, sb, st, sh, sw, sc, nclip, T, pad, FH, FW, S, h->stream); }));
    Epi e;
    e.relu = 1; e.scale = src_u8 ? h->gs.c1_scale255 : nullptr; e.out16 = o1;
    RET(gemm(h, JG_ST_CONV1, S, 0, (int)(NF * 88 * 158), h->gs.c1, e, &g[0]));
    return timed(h, JG_ST_POOL, [&] { return LAUNCH(h, launch_maxpool3x3s2, o1, pooled, (int)NF, 88, 158, 64, h->stream, nullptr, 0, nullptr); });
}

// conv stack over `nclip` temporal volumes -> conv_out (nclip*P, 512) fp32, P = T + 2*pad - 4
// conv16 (optional): fp16 copy of conv_out, the A operand of the per-position qkv projection (gs_transformer, Qkv0)
static int gs_conv_stack(jg_handle* h, const void* src, int src_u8, long sb, long st, long sh, long sw, long sc,
                         int nclip, int T, int pad, float* conv_out, f16* conv16 = nullptr) {
    const GestSyncModel& gs = h->gs;
    const int P = T + 2 * pad - 4;
    const long NF = (long)nclip * P;
    f16 *p1, *o2, *o3, *o4, *o5, *p5;
    const int* s2pos = nullptr;          // per-position row-skip counts (direct path with conv2_row_skip)
    ConvGeom g[5];
    gs_conv_geoms(g);
    RET(wsalloc(h, (size_t)NF * 43 * 78 * 64, &p1));
    RET(wsalloc(h, (size_t)NF * 20 * 37 * 128, &o2));
    RET(wsalloc(h, (size_t)NF * 10 * 19 * 256, &o3));
    RET(wsalloc(h, (size_t)NF * 10 * 10 * 256, &o4));
    RET(wsalloc(h, (size_t)NF * 10 * 10 * 256, &o5));
    RET(wsalloc(h, (size_t)NF * 4 * 4 * 256, &p5));
    // Position-independent leading rows (common.h, ConvGeom::rowmap): the zero-band scan of the direct conv1 leaves every position's
    // count s2 in zscr; conv2 .. conv5 leave those rows out PER POSITION (compacted row maps built on the device) and conv3 .. conv5 and
    // the last max-pool read them from the const chain.  Only the LDS-DMA conv kernel knows how, so every layer of the chain must
    // take that path: the planner is asked about conv2 .. conv5 of this launch with a row map.
    const Lin* cl[4] = {&gs.c2, &gs.c3, &gs.c4, &gs.c5};
    bool rowskip = h->opts.conv1_zero_skip && h->conv2_row_skip && gs.c2C;
    for (int l = 0; l < 4 && rowskip; ++l) {
        GemmShape q = {};
        q.set_geom(g[l + 1]);
        q.rowmap = true; q.const_in = l > 0;
        q.M = NF * g[l + 1].OH * g[l + 1].OW; q.N = cl[l]->N; q.K = q.ldw = cl[l]->K; q.ldc = cl[l]->N;
        q.w2 = run_lo(h, *cl[l], false) != nullptr; q.bias = q.out16 = true; q.relu = 1;
        rowskip = plan_gemm(q, h->opts).glds();
    }
    unsigned* zscr;
    RET(gs_conv1_stage(h, src, src_u8, sb, st, sh, sw, sc, nclip, T, pad, p1, !rowskip, &zscr));
    if (zscr && rowskip) {
        s2pos = conv1_s2_counts(zscr, nclip, T, pad);
        const f16* cin[4] = {nullptr, gs.c2C, gs.c3C, gs.c4C};
        ConvRowMap rm[4];
        int OH[4], OW[4];
        for (int l = 0; l < 4; ++l) {
            OH[l] = g[l + 1].OH; OW[l] = g[l + 1].OW;
            h->conv_report.full[l] = NF * OH[l] * OW[l];
        }
        RET(rowmap_chain(h, NF, 4, OH, OW, 0, rm, g + 1, cin));
        RET(timed(h, JG_ST_CONV1_AUX, [&] { return launch_conv_rowmaps(s2pos, (int)NF, rm, 4, h->stream); }));
        h->conv_report.totals = rm[0].total;
        h->conv_report.rowskip = conv1_scan_view(zscr, nclip, T, pad).rowskip_min();
    }
    Epi e;
    e.relu = 1;
    e.out16 = o2; RET(gemm(h, JG_ST_CONV, p1, 0, (int)(NF * 20 * 37), gs.c2, e, &g[1]));
    e.out16 = o3; RET(gemm(h, JG_ST_CONV, o2, 0, (int)(NF * 10 * 19), gs.c3, e, &g[2]));
    e.out16 = o4; RET(gemm(h, JG_ST_CONV, o3, 0, (int)(NF * 10 * 10), gs.c4, e, &g[3]));
    e.out16 = o5; RET(gemm(h, JG_ST_CONV, o4, 0, (int)(NF * 10 * 10), gs.c5, e, &g[4]));
    RET(timed(h, JG_ST_POOL, [&] { return LAUNCH(h, launch_maxpool3x3s2, o5, p5, (int)NF, 10, 10, 256, h->stream, s2pos, 3, gs.c5C); }));
    e.out16 = conv16; e.out32 = conv_out;
    return gemm(h, JG_ST_CONV, p5, 4096, (int)NF, gs.fc6, e);
}

// post-norm transformer (gestsync.py:20-21) in place on x32/x16, M = nseq*21 tokens
// Whether the whole GestSync transformer of M tokens runs with residual+LayerNorm fused into the projection GEMMs.
// All twelve projections must qualify (single-fp16 weights, not the calibration pass): the fused kernel keeps the
// fp32 residual stream in its own tiled order (gemm.hip), so fused and unfused layers cannot be mixed.
// rows_per_clip: rows of one clip in the launch (T * 21 on the clip path; 0: no clip structure, e.g. forward_vid windows).  In the
// run-time corrected mode the LayerNorm-fused projections exist with the per-clip bias only (there is no hi+lo instance of that
// kernel), so there the questions are asked in the per-clip-bias form: clips too short for it (T <= 12) and launches without clip
// structure take the unfused plan, whose GEMMs run hi+lo (such batches used to fail with hipErrorInvalidValue).
// Policy here: the option, not calibrating, the fp16 build (the token stream is fp16), no lo operand behind a fused LayerNorm (asked
// in the per-clip-bias form, the one these launches take: a run-time corrected layer answers "none").
// Shape: the planner accepts all four GEMM kinds of a layer at this M -- qkv and linear1 on the tiled token plane, out_proj and
// linear2 with the LayerNorm fused.
static bool gs_fused_plan(const jg_handle* h, int M, int rows_per_clip) {
    if (!h->fuse_ln || h->calib || h->bf16) return false;
    for (int l = 0; l < 6; ++l)
        if (run_lo(h, h->gs.layers[l].out, true) || run_lo(h, h->gs.layers[l].ff2, true)) return false;
    const bool clip_bias = h->precision == JG_PREC_FP16_RC;
    auto plans = [&](int N, int K, bool ln, int relu) {
        GemmShape q = {};
        q.M = M; q.N = q.ldc = N; q.K = q.lda = q.ldw = K;
        q.bias = q.out16 = true; q.relu = relu;
        q.a_tiled = !ln; q.ln_w = q.res16 = ln;
        if (clip_bias) { q.bias_clip = true; q.rpc = rows_per_clip; q.nclips = rows_per_clip > 0 ? M / rows_per_clip : 0; }
        return plan_gemm(q, h->opts).ok();
    };
    return plans(1536, 512, false, 0) && plans(512, 512, true, 0) && plans(2048, 512, false, 1) && plans(512, 2048, true, 0);
}

// x32/x16 hold pad128(M) rows.  With `tiled` (gs_fused_plan) the token stream is the tiled fp16 plane x16 alone (x32 is not
// used); otherwise fp32 rows + fp16 rows.
// Layer 0's qkv projection by linearity (clip path): token j of window (clip c, frame i) is conv[c][clamp(i+j-shift)] + pe[j],
// so W x + b = W conv[c][p] + (W pe[j] + b).  The projection then runs over the nclip*P distinct conv positions (154 per clip
// instead of 150 * 21 tokens) plus the 21 positional rows, and the attention kernel gathers and sums the operand rows
// (attention.hip, attn_mfma_s32_kernel<true>): no 310 MB qkv tensor for layer 0.
struct Qkv0 {
    const f16* conv16;    // [nclip*P][512]
    int nclip, P, Twin, shift;
};

// The unfused plan: six post-norm layers (post_norm_layer, engine.h) on the stream x32 with its operand copy x (T = float: x32 itself).
// t32: the projections' fp32 output -- the 16-bit plan runs in place (t32 = x32), the audit path through a buffer of its own
template <class T>
static int gs_layers(jg_handle* h, Arith<T> ar, float* x32, T* x, float* t32, int nseq, int S) {
    const int M = nseq * S;
    T *qkv, *att, *hid;
    RET(wsalloc(h, (size_t)M * 1536, &qkv));
    RET(wsalloc(h, (size_t)M * 512, &att));
    RET(wsalloc(h, (size_t)M * 2048, &hid));
    for (int l = 0; l < 6; ++l) RET(post_norm_layer(h, ar, h->gs.layers[l], x32, x, t32, qkv, att, hid, nullptr, nseq, S, 8, 512, 2048, 1, x32));
    return JG_OK;
}

// The fused plan (gs_fused_plan) stays a graph of its own: its token stream is the tiled fp16 plane x16 alone, out_proj / linear2 carry the
// residual add and the post-norm LayerNorm in their epilogues (row-wide 128x512 tiles), and layer 0 may take its qkv by linearity (Qkv0) --
// none of which exists in fp32 or bf16.  rc_clips > 0: the rows are rc_clips clips of M / rc_clips rows each (the clip path;
// JG_PREC_FP16_RC's per-clip corrections)
static int gs_transformer(jg_handle* h, float* x32, f16* x16, int nseq, int S, bool tiled, const Qkv0* q0 = nullptr, int rc_clips = 0,
                          const int* rc_valid = nullptr) {
    if (!tiled) return gs_layers(h, A16(), x32, x16, x32, nseq, S);
    GestSyncModel& gs = h->gs;
    const int M = nseq * S;
    const int rc_rpc = rc_clips > 0 ? M / rc_clips : 0;
    f16 *qkv, *att, *hid;
    RET(wsalloc(h, (size_t)M * 1536, &qkv));
    RET(wsalloc(h, (size_t)M * 512, &att));
    RET(wsalloc(h, (size_t)M * 2048, &hid));
    Epi e, r, f;
    e.out16 = qkv; e.a_tiled = 1; e.rc_rpc = rc_rpc; e.rc_clips = rc_clips; e.rc_valid = rc_valid;
    r.res16 = x16; r.out16 = x16; r.ln_flavour = LN_STD; r.rc_rpc = rc_rpc; r.rc_clips = rc_clips; r.rc_valid = rc_valid;
    f = e; f.relu = 1; f.out16 = hid;
    for (int l = 0; l < 6; ++l) {
        const EncLayer& L = gs.layers[l];
        if (l == 0 && q0) {
            f16* qpos;
            RET(wsalloc(h, (size_t)q0->nclip * q0->P * 1536, &qpos));
            if (!gs.qpe) RET(walloc(h, gs.m, (size_t)32 * 1536, &gs.qpe));
            f16* qpe = gs.qpe;
            Epi p;
            p.out16 = qpos; p.no_bias = 1;
            RET(gemm(h, JG_ST_GEMM, q0->conv16, 512, q0->nclip * q0->P, L.qkv, p));
            if (!gs.qpe_valid) {
                RET(timed(h, JG_ST_GEMM, [&] { return launch_pe_project(gs.pe, S, L.qkv.wh, run_lo(h, L.qkv, false), L.qkv.bias, 1536, 512, qpe, h->stream); }));
                HIPCHK(h, hipStreamSynchronize(h->stream));      // once per weight load: later calls may come on another stream
                gs.qpe_valid = true;
            }
            const AttnGather ag = {qpe, q0->Twin, q0->P, q0->shift};
            RET(timed(h, JG_ST_ATTN, [&] { return launch_attention_gather(qpos, ag, nseq, S, 8, att, h->stream); }));
        } else {
            RET(gemm(h, JG_ST_GEMM, x16, 512, M, L.qkv, e));
            RET(attention(h, A16(), qkv, nullptr, nseq, S, 8, 64, att));
        }
        r.ln = &L.n1; RET(gemm(h, JG_ST_GEMM, att, 512, M, L.out, r));
        RET(gemm(h, JG_ST_GEMM, x16, 512, M, L.ff1, f));
        r.ln = &L.n2; RET(gemm(h, JG_ST_GEMM, hid, 2048, M, L.ff2, r));
    }
    return JG_OK;
}

// ------------------------------------------------------------------------------------ fp32 audit path (audit32.hip)
// JG_PREC_FP32 (and option audit_stages on a handle finalized with audit_weights): the same stages as above on fp32 weights and fp32
// activations, exact-fp32 MFMAs, fp32 softmax / LayerNorm.  The reference's CPU path is fp32 (inference_embs.py:497 -- autocast does nothing
// without CUDA): this is the on-device stand-in for it, what the fp16 modes are audited against on a checkpoint the parity tests never saw.
// Straightforward on purpose (no window de-duplication tricks beyond the distinct conv positions, no fused epilogues beyond bias /
// residual / activation, the mean(-1) AFTER ff_vid.2 as in inference_embs.py:511); ~40-60 clips/s.

// conv stack over `nclip` temporal volumes -> conv_out (nclip*P, 512) fp32 (gestsync.py:34-87,308-325: conv + BatchNorm(eval, folded) + ReLU, two max-pools)
// A graph of its own next to gs_conv_stack: that one is the direct u8 conv1 with its zero-band scan and the row-skip chain behind it, this
// one the plain chain of seven layers -- they share the geometry (gs_conv_geoms) and nothing else.
static int gs_conv_stack32(jg_handle* h, const void* src, int src_u8, long sb, long st, long sh, long sw, long sc, int nclip, int T, int pad, float* conv_out) {
    const GestSyncModel& gs = h->gs;
    const int P = T + 2 * pad - 4;
    const long NF = (long)nclip * P;
    if (NF * 88 * 158 >= (1L << 31)) JG_FAIL(h, JG_ERR_ARG, "fp32 conv stack: too many positions in one pass (lower jg_set_chunk)");
    ConvGeom g[5];
    gs_conv_geoms(g);
    float *S, *o1, *p1, *o2, *o3, *o4, *o5, *p5;
    RET(wsalloc(h, (size_t)NF * FH * FW * 16, &S));
    RET(wsalloc(h, (size_t)NF * 88 * 158 * 64, &o1));
    RET(wsalloc(h, (size_t)NF * 43 * 78 * 64, &p1));
    RET(wsalloc(h, (size_t)NF * 20 * 37 * 128, &o2));
    RET(wsalloc(h, (size_t)NF * 10 * 19 * 256, &o3));
    RET(wsalloc(h, (size_t)NF * 10 * 10 * 256, &o4));
    RET(wsalloc(h, (size_t)NF * 10 * 10 * 256, &o5));
    RET(wsalloc(h, (size_t)NF * 4 * 4 * 256, &p5));
    RET(timed(h, JG_ST_STACK, [&] { return launch_stack_frames32(src, src_u8, sb, st, sh, sw, sc, nclip, T, pad, FH, FW, S, h->stream); }));
    Epi32 e;
    e.act = 1;
    RET(gemm32(h, JG_ST_CONV1, S, 0, (int)(NF * 88 * 158), gs.c1, o1, e, &g[0]));
    RET(timed(h, JG_ST_POOL, [&] { return launch_maxpool3x3s2_32(o1, p1, (int)NF, 88, 158, 64, h->stream); }));
    RET(gemm32(h, JG_ST_CONV, p1, 0, (int)(NF * 20 * 37), gs.c2, o2, e, &g[1]));
    RET(gemm32(h, JG_ST_CONV, o2, 0, (int)(NF * 10 * 19), gs.c3, o3, e, &g[2]));
    RET(gemm32(h, JG_ST_CONV, o3, 0, (int)(NF * 10 * 10), gs.c4, o4, e, &g[3]));
    RET(gemm32(h, JG_ST_CONV, o4, 0, (int)(NF * 10 * 10), gs.c5, o5, e, &g[4]));
    RET(timed(h, JG_ST_POOL, [&] { return launch_maxpool3x3s2_32(o5, p5, (int)NF, 10, 10, 256, h->stream); }));
    return gemm32(h, JG_ST_CONV, p5, 4096, (int)NF, gs.fc6, conv_out, e);
}

// windows + PE + transformer + ff_vid on the fp32 kernels: conv (nb*P, 512) fp32 -> *full (nb*T*21, 1024), T windows per volume
// The tail is not shared with the 16-bit clip path on purpose: that one takes the window mean BEFORE ff_vid.2 (by linearity, 21 x fewer
// rows), the audit path after it, as the reference does.
static int gs_tail32(jg_handle* h, const float* conv, int nb, int P, int T, int shift, float** full) {
    const int S = 21, nseq = nb * T, M = nseq * S;
    float *x32, *t32, *hid;
    RET(wsalloc(h, (size_t)M * 512, &x32));
    RET(wsalloc(h, (size_t)M * 512, &t32));
    RET(timed(h, JG_ST_MISC, [&] { return launch_window_gather(conv, h->gs.pe, nb, P, T, S, 512, shift, 0, x32, nullptr, h->stream); }));
    RET(gs_layers(h, A32(), x32, x32, t32, nseq, S));
    RET(wsalloc(h, (size_t)M * 512, &hid));
    RET(wsalloc(h, (size_t)M * 1024, full));
    Epi32 f; f.act = 1;
    RET(gemm32(h, JG_ST_GEMM, x32, 512, M, h->gs.ff0, hid, f));
    return gemm32(h, JG_ST_GEMM, hid, 512, M, h->gs.ff2, *full);
}

// valid_host (optional, host [B]): clip b's first valid_host[b] frames are its own, the rest of its T frames is batch padding (copies of its
// last frame, jg_gestsync_clip_ragged): only the run-time corrected mode looks at it -- a clip's statistics come from its own rows
int gestsync_clip_impl(jg_handle* h, const void* frames, int dtype, int B, int T, float* out_feats, const int32_t* valid_host) {
    if (!h->gs.m.ready) JG_FAIL(h, JG_ERR_STATE, "GestSync weights not finalized");
    if (B <= 0 || T <= 0) JG_FAIL(h, JG_ERR_ARG, "B and T must be positive");
    if (dtype != JG_U8 && dtype != JG_F32) JG_FAIL(h, JG_ERR_ARG, "frames dtype must be JG_U8 or JG_F32");
    // Edge padding 12 (inference_embs.py:283) gives T+20 conv positions, but positions 0..8 and
    // T+11..T+19 each see five copies of one frame: evaluate the T+4 distinct ones (== padding 4) and
    // let the window gather clamp.  Bit-identical to evaluating all T+20.
    const int PAD = h->edge_dedup ? 4 : 12;
    const int P = T + 2 * PAD - 4, S = 21;
    const size_t esz = dtype == JG_U8 ? 1 : 4;
    const long sw = 3, sh = (long)FW * 3, st = (long)FH * FW * 3, sb = (long)T * st;
    // fp32 audit stages (audit_mask): the conv stack and / or the transformer + ff_vid of this call run on the fp32 kernels; a pass of the
    // fp32 conv stack holds 2.1 GB per 150-frame clip, so its passes are two clips
    const int am = audit_mask(h);
    const int chunk = (am & AUD_CONV) ? std::min(h->chunk, 2) : h->chunk;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        RET(begin_pass(h));
        float* conv;
        RET(wsalloc(h, (size_t)nb * P * 512, &conv));
        const char* src = reinterpret_cast<const char*>(frames) + (size_t)b0 * sb * esz;
        const int nseq = nb * T, M = nseq * S;
        float* x32; f16 *x16, *hid, *mean16, *conv16 = nullptr;
        const bool tiled = !(am & AUD_GS) && gs_fused_plan(h, M, T * S);
        int* rc_valid = nullptr;
        if (valid_host && tiled && h->precision == JG_PREC_FP16_RC) {
            std::vector<int32_t> hv(nb);
            for (int b = 0; b < nb; ++b) hv[b] = valid_host[b0 + b] * S;              // rows = frames x 21 tokens
            RET(wsalloc(h, (size_t)nb, &rc_valid));
            RET(upload_i32_async(h, hv.data(), (size_t)nb, rc_valid));
        }
        // layer-0 qkv from the distinct conv positions: worth it when the windows overlap (T > 1) and the MFMA attention runs
        const bool lin0 = tiled && h->qkv0_linear && h->opts.attn_mfma && T > 1;
        if (lin0) RET(wsalloc(h, (size_t)nb * P * 512, &conv16));
        if (am & AUD_CONV) {
            RET(gs_conv_stack32(h, src, dtype == JG_U8, sb, st, sh, sw, 1, nb, T, PAD, conv));
            if (conv16) RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_cast_f32_f16, (const float*)conv, conv16, (long)nb * P * 512, h->stream); }));
        } else {
            RET(gs_conv_stack(h, src, dtype == JG_U8, sb, st, sh, sw, 1, nb, T, PAD, conv, conv16));
        }
        if (am & AUD_GS) {
            float* full;
            RET(gs_tail32(h, conv, nb, P, T, 12 - PAD, &full));
            RET(timed(h, JG_ST_MISC, [&] { return launch_group_mean32(full, nseq, S, 1024, out_feats + (size_t)b0 * T * 1024, h->stream); }));
            continue;
        }
        RET(wsalloc(h, pad128(M) * 512, &x32));
        RET(wsalloc(h, pad128(M) * 512, &x16));
        RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_window_gather, conv, h->gs.pe, nb, P, T, S, 512, 12 - PAD, tiled, x32, x16, h->stream); }));
        const Qkv0 q0 = {conv16, nb, P, T, 12 - PAD};
        RET(gs_transformer(h, x32, x16, nseq, S, tiled, lin0 ? &q0 : nullptr, nb, rc_valid));
        RET(wsalloc(h, (size_t)M * 512, &hid));
        RET(wsalloc(h, (size_t)nseq * 512, &mean16));
        Epi f; f.relu = 1; f.out16 = hid; f.a_tiled = tiled;
        if (tiled) { f.rc_rpc = T * S; f.rc_clips = nb; f.rc_valid = rc_valid; }
        RET(gemm(h, JG_ST_GEMM, x16, 512, M, h->gs.ff0, f));
        RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_group_mean, hid, nseq, S, 512, mean16, h->stream); }));
        Epi o; o.out32 = out_feats + (size_t)b0 * T * 1024;
        RET(gemm(h, JG_ST_GEMM, mean16, 512, nseq, h->gs.ff2, o));
    }
    return JG_OK;
}

int gestsync_windows_impl(jg_handle* h, const float* x, int N, float* out, float* out_conv) {
    if (!h->gs.m.ready) JG_FAIL(h, JG_ERR_STATE, "GestSync weights not finalized");
    if (N <= 0) JG_FAIL(h, JG_ERR_ARG, "N must be positive");
    const int S = 21;
    const long sw = 1, sh = FW, st = (long)FH * FW, sc = 25 * st, sb = 3 * sc;
    const int am = audit_mask(h);
    const int wchunk = (am & AUD_CONV) ? 16 : std::max(1, h->chunk * 8);      // (fp32 conv stack: 0.26 GB per window)
    for (int n0 = 0; n0 < N; n0 += wchunk) {
        const int nb = std::min(wchunk, N - n0);
        RET(begin_pass(h));
        float* conv;
        RET(wsalloc(h, (size_t)nb * S * 512, &conv));
        if (am & AUD_CONV) RET(gs_conv_stack32(h, x + (size_t)n0 * sb, 0, sb, st, sh, sw, sc, nb, 25, 0, conv));
        else RET(gs_conv_stack(h, x + (size_t)n0 * sb, 0, sb, st, sh, sw, sc, nb, 25, 0, conv));
        if (out_conv)
            RET(timed(h, JG_ST_MISC, [&] { return launch_transpose_tokens(conv, nb, S, 512, out_conv + (size_t)n0 * 512 * S, h->stream); }));
        const int M = nb * S;
        float* full;
        if (am & AUD_GS) {
            RET(gs_tail32(h, conv, nb, S, 1, 0, &full));
        } else {
            float* x32; f16 *x16, *hid;
            const bool tiled = gs_fused_plan(h, M, 0);
            RET(wsalloc(h, pad128(M) * 512, &x32));
            RET(wsalloc(h, pad128(M) * 512, &x16));
            RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_window_gather, conv, h->gs.pe, nb, S, 1, S, 512, 0, tiled, x32, x16, h->stream); }));
            RET(gs_transformer(h, x32, x16, nb, S, tiled));
            RET(wsalloc(h, (size_t)M * 512, &hid));
            RET(wsalloc(h, (size_t)M * 1024, &full));
            Epi f; f.relu = 1; f.out16 = hid; f.a_tiled = tiled;
            RET(gemm(h, JG_ST_GEMM, x16, 512, M, h->gs.ff0, f));
            Epi o; o.out32 = full;
            RET(gemm(h, JG_ST_GEMM, hid, 512, M, h->gs.ff2, o));
        }
        RET(timed(h, JG_ST_MISC, [&] { return launch_transpose_tokens(full, nb, S, 1024, out + (size_t)n0 * 1024 * S, h->stream); }));
    }
    return JG_OK;
}

}  // namespace engine
