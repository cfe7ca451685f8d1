// libjegal_hip: XLM-RoBERTa, the text front end -- finalize, the folded pass, the unfolded pass per arithmetic.  Host code only.
#include "engine.h"
#include <type_traits>

namespace engine {

namespace {
constexpr int D = 768, DFF = 3072, H = 12;          // xlm-roberta-base: hidden size, intermediate size, heads of 64
}  // namespace

// State-dict keys: those of transformers.XLMRobertaModel (add_pooling_layer irrelevant) under the prefix "xlmr.":
// xlmr.embeddings.{word,position,token_type}_embeddings.weight, xlmr.embeddings.LayerNorm.{weight,bias},
// xlmr.encoder.layer.<i>.attention.self.{query,key,value}.{weight,bias}, .attention.output.{dense,LayerNorm}.*,
// .intermediate.dense.*, .output.{dense,LayerNorm}.*.  The number of layers is the number present; hidden size 768,
// 12 heads of 64, intermediate 3072 (xlm-roberta-base); the vocabulary and position table sizes come from the tensors.
int finalize_xlmr(jg_handle* h) {
    drop_model(h, h->xl);          // frees the previous weights, drops its bias-corrected layers
    XlmrModel& xl = h->xl;
    Model& m = xl.m;
    const HostTensor* t = find(h, "xlmr.embeddings.word_embeddings.weight");
    if (!t || t->numel() % D) JG_FAIL(h, JG_ERR_WEIGHT, "missing or malformed 'xlmr.embeddings.word_embeddings.weight'");
    xl.vocab = (int)(t->numel() / D);
    RET(upload(h, m, t->v, &xl.word));
    t = find(h, "xlmr.embeddings.position_embeddings.weight");
    if (!t || t->numel() % D) JG_FAIL(h, JG_ERR_WEIGHT, "missing or malformed 'xlmr.embeddings.position_embeddings.weight'");
    xl.maxpos = (int)(t->numel() / D);
    RET(upload(h, m, t->v, &xl.pos));
    RET(need(h, "xlmr.embeddings.token_type_embeddings.weight", D, &t));
    RET(upload(h, m, t->v, &xl.type));
    RET(make_ln(h, m, "xlmr.embeddings.LayerNorm.weight", "xlmr.embeddings.LayerNorm.bias", D, &xl.emb_ln));
    // Implicit LayerNorm (xlmr_encode_folded): the Linear BEHIND a LayerNorm(gamma, beta) is packed as W diag(gamma) with bias
    // b + W beta (fold_ln_consumer, weight_pack.h), the Linear whose output is ADDED to that LayerNorm's output takes beta into its bias (the
    // gamma (x - mean) rstd part is recomputed from the un-normalised stream in its epilogue).
    // (the implicit-LayerNorm epilogues exist in the LDS-DMA kernel only -- plan_gemm, gemm_plan.hip; the option is the policy here, the
    // packing happens before any shape is known.  The fp32 audit path runs the explicit LayerNorms on the un-folded matrices, so audit
    // weights switch the folding off)
    const bool fold = h->xl_fold_opt && h->opts.gemm_glds && !h->audit_weights && h->precision != JG_PREC_FP32;
    const HostTensor *pg, *pb;          // the LayerNorm in front of the current sub-layer
    RET(need(h, "xlmr.embeddings.LayerNorm.weight", D, &pg));
    RET(need(h, "xlmr.embeddings.LayerNorm.bias", D, &pb));
    auto make_producer = [&](const std::string& wname, const std::string& bname, int N, int K, const std::vector<float>& be, Lin* Lo) -> int {
        const HostTensor *w, *b;
        RET(need(h, wname, (int64_t)N * K, &w));
        RET(need(h, bname, N, &b));
        std::vector<float> bb = b->v;
        fold_ln_producer(bb.data(), N, be.data());
        return pack_matrix(h, m, w->v, bb, N, K, LK_XLMR, Lo);
    };
    int nl = 0;
    while (find(h, "xlmr.encoder.layer." + std::to_string(nl) + ".attention.self.query.weight")) ++nl;
    if (nl == 0) JG_FAIL(h, JG_ERR_WEIGHT, "no 'xlmr.encoder.layer.*' weights");
    xl.layers.resize(nl);
    for (int l = 0; l < nl; ++l) {
        const std::string p = "xlmr.encoder.layer." + std::to_string(l);
        EncLayer* L = &xl.layers[l];
        std::vector<float> w((size_t)3 * D * D), b((size_t)3 * D);
        const char* names[3] = {"query", "key", "value"};
        for (int i = 0; i < 3; ++i) {
            const HostTensor *wi, *bi;
            RET(need(h, p + ".attention.self." + names[i] + ".weight", (int64_t)D * D, &wi));
            RET(need(h, p + ".attention.self." + names[i] + ".bias", D, &bi));
            std::memcpy(&w[(size_t)i * D * D], wi->v.data(), sizeof(float) * D * D);
            std::memcpy(&b[(size_t)i * D], bi->v.data(), sizeof(float) * D);
        }
        if (!fold) {
            RET(pack_matrix(h, m, w, b, 3 * D, D, LK_XLMR, &L->qkv));
            RET(make_linear(h, m, p + ".attention.output.dense.weight", p + ".attention.output.dense.bias", D, D, &L->out, LK_XLMR));
            RET(make_ln(h, m, p + ".attention.output.LayerNorm.weight", p + ".attention.output.LayerNorm.bias", D, &L->n1));
            RET(make_linear(h, m, p + ".intermediate.dense.weight", p + ".intermediate.dense.bias", DFF, D, &L->ff1, LK_XLMR));
            RET(make_linear(h, m, p + ".output.dense.weight", p + ".output.dense.bias", D, DFF, &L->ff2, LK_XLMR));
            RET(make_ln(h, m, p + ".output.LayerNorm.weight", p + ".output.LayerNorm.bias", D, &L->n2));
            continue;
        }
        fold_ln_consumer(w.data(), b.data(), 3 * D, D, pg->v.data(), pb->v.data());
        RET(pack_matrix(h, m, w, b, 3 * D, D, LK_XLMR, &L->qkv, true));
        RET(make_producer(p + ".attention.output.dense.weight", p + ".attention.output.dense.bias", D, D, pb->v, &L->out));
        RET(make_ln(h, m, p + ".attention.output.LayerNorm.weight", p + ".attention.output.LayerNorm.bias", D, &L->n1));
        RET(need(h, p + ".attention.output.LayerNorm.weight", D, &pg));
        RET(need(h, p + ".attention.output.LayerNorm.bias", D, &pb));
        {
            const HostTensor *w1, *b1;
            RET(need(h, p + ".intermediate.dense.weight", (int64_t)DFF * D, &w1));
            RET(need(h, p + ".intermediate.dense.bias", DFF, &b1));
            std::vector<float> wf = w1->v, bf1 = b1->v;
            fold_ln_consumer(wf.data(), bf1.data(), DFF, D, pg->v.data(), pb->v.data());
            RET(pack_matrix(h, m, wf, bf1, DFF, D, LK_XLMR, &L->ff1, true));
        }
        RET(make_producer(p + ".output.dense.weight", p + ".output.dense.bias", D, DFF, pb->v, &L->ff2));
        RET(make_ln(h, m, p + ".output.LayerNorm.weight", p + ".output.LayerNorm.bias", D, &L->n2));
        RET(need(h, p + ".output.LayerNorm.weight", D, &pg));
        RET(need(h, p + ".output.LayerNorm.bias", D, &pb));
    }
    xl.folded = fold;
    m.ready = true;
    return JG_OK;
}

// XLMRobertaModel.forward with explicit LayerNorms on un-folded matrices (option xlmr_fold = 0; finalize_xlmr also packs them that way
// when audit weights are kept): embeddings + LayerNorm, then post-norm BERT layers (post_norm_layer, engine.h) with exact GELU
template <class T>
static int xlmr_encode_unfolded(jg_handle* h, Arith<T> ar, const int32_t* ids, const int32_t* amask, int B, int L, float* out) {
    const XlmrModel& xl = h->xl;
    const int M = B * L;
    float *x32, *t32, *mk = nullptr;
    T *x, *qkv, *att, *hid;
    RET(wsalloc(h, (size_t)M * D, &x32));
    if constexpr (std::is_same<T, float>::value) x = x32; else RET(wsalloc(h, (size_t)M * D, &x));
    RET(wsalloc(h, (size_t)M * D, &t32));
    RET(wsalloc(h, (size_t)M * 3 * D, &qkv));
    RET(wsalloc(h, (size_t)M * D, &att));
    RET(wsalloc(h, (size_t)M * DFF, &hid));
    if (amask) {
        RET(wsalloc(h, (size_t)M, &mk));
        RET(timed(h, JG_ST_MISC, [&] { return launch_mask_i32_f32(amask, mk, M, h->stream); }));
    }
    RET(timed(h, JG_ST_MISC, [&] { return launch_xlmr_embed(ids, B, L, D, 1, xl.vocab, xl.maxpos, xl.word, xl.pos, xl.type, t32, h->stream); }));
    RET(layernorm(h, ar, t32, xl.emb_ln, M, D, LN_STD, 0, x, x32));
    const int n = (int)xl.layers.size();
    for (int l = 0; l < n; ++l) RET(post_norm_layer(h, ar, xl.layers[l], x32, x, t32, qkv, att, hid, mk, B, L, H, D, DFF, 2, l + 1 == n ? out : x32));
    return JG_OK;
}

// XLMRobertaModel.forward(input_ids, attention_mask).last_hidden_state: post-norm BERT layers (LayerNorm eps 1e-5, exact GELU),
// the key padding mask of attention_mask, position ids from the non-pad tokens (padding_idx = 1).
// The same forward pass with IMPLICIT LayerNorms (option xlmr_fold, default): post-norm layers x' = LN(x + f(x)) are carried as the
// UN-normalised sums x (two fp16 planes hi + lo; hi is the next GEMM's A operand) plus (mean, rstd) per row.  A Linear behind a
// LayerNorm runs on x with W diag(gamma) and finishes rstd (acc - mean c1) + (b + W beta) in its epilogue; a Linear whose output is
// added to LN(x) recomputes gamma (x - mean) rstd + beta from the planes there, writes the new planes in place and the per-64-column
// (sum, sum of squares) of the new rows; launch_ln_stats (one thread per row) makes the next (mean, rstd).  Per pass: 25 LayerNorm
// launches over fp32 rows (10 % of the time, 18 B per element and sub-layer through HBM) become 24 x 3 us and 8 B per element.
// A graph of its own: no LayerNorm launch, no fp32 stream and no operand copy exist here, and only the 16-bit LDS-DMA GEMM has its epilogues.
static int xlmr_encode_folded(jg_handle* h, const int32_t* ids, const int32_t* amask, int B, int L, float* out) {
    const XlmrModel& xl = h->xl;
    constexpr int P = D / 64;
    const int M = B * L;
    const int Mp = M < GEMM_GLDS_MIN_ROWS ? GEMM_GLDS_MIN_ROWS : M;      // the LDS-DMA GEMMs' minimum (gemm_plan.h): short batches carry zero rows behind the tokens
    float *part, *stats, *mk = nullptr;
    f16 *xh, *xlo, *qkv, *att, *hid;
    RET(wsalloc(h, (size_t)Mp * D, &xh));
    RET(wsalloc(h, (size_t)Mp * D, &xlo));
    RET(wsalloc(h, (size_t)Mp * P * 2, &part));
    RET(wsalloc(h, (size_t)Mp * 2, &stats));
    RET(wsalloc(h, (size_t)Mp * 3 * D, &qkv));
    RET(wsalloc(h, (size_t)Mp * D, &att));
    RET(wsalloc(h, (size_t)Mp * DFF, &hid));
    if (Mp > M) {
        HIPCHK(h, hipMemsetAsync(xh + (size_t)M * D, 0, (size_t)(Mp - M) * D * sizeof(f16), h->stream));
        HIPCHK(h, hipMemsetAsync(xlo + (size_t)M * D, 0, (size_t)(Mp - M) * D * sizeof(f16), h->stream));
        HIPCHK(h, hipMemsetAsync(part + (size_t)M * P * 2, 0, (size_t)(Mp - M) * P * 2 * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(att + (size_t)M * D, 0, (size_t)(Mp - M) * D * sizeof(f16), h->stream));
    }
    if (amask) {
        RET(wsalloc(h, (size_t)M, &mk));
        RET(timed(h, JG_ST_MISC, [&] { return launch_mask_i32_f32(amask, mk, M, h->stream); }));
    }
    RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_xlmr_embed_planes, ids, B, L, D, 1, xl.vocab, xl.maxpos, xl.word, xl.pos, xl.type, xh, xlo, part, h->stream); }));
    auto ln_stats = [&]() { return timed(h, JG_ST_NORM, [&] { return launch_ln_stats(part, Mp, P, stats, h->stream); }); };
    RET(ln_stats());
    const LNp* prev = &xl.emb_ln;
    for (int l = 0; l < (int)xl.layers.size(); ++l) {
        const EncLayer& Ly = xl.layers[l];
        Epi q; q.out16 = qkv; q.ln_mode = 1; q.ln_stats = stats; q.calib_rows = M;
        RET(gemm(h, JG_ST_GEMM, xh, D, Mp, Ly.qkv, q));
        RET(timed(h, JG_ST_ATTN, [&] { return LAUNCH(h, launch_attention, qkv, mk, B, L, H, 64, att, h->opts, h->stream); }));
        Epi o; o.ln_mode = 2; o.ln_stats = stats; o.x_hi = xh; o.x_lo = xlo; o.ln_gamma = prev->w; o.stat_out = part; o.calib_rows = M;
        RET(gemm(h, JG_ST_GEMM, att, D, Mp, Ly.out, o));
        RET(ln_stats());
        Epi f; f.relu = 2; f.out16 = hid; f.ln_mode = 1; f.ln_stats = stats; f.calib_rows = M;
        RET(gemm(h, JG_ST_GEMM, xh, D, Mp, Ly.ff1, f));
        o.ln_gamma = Ly.n1.w;
        RET(gemm(h, JG_ST_GEMM, hid, DFF, Mp, Ly.ff2, o));
        if (l + 1 < (int)xl.layers.size()) RET(ln_stats());
        prev = &Ly.n2;
    }
    return timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm_planes, xh, xlo, prev->w, prev->b, M, D, out, h->stream); });
}

int xlmr_encode_impl(jg_handle* h, const int32_t* ids, const int32_t* amask, int B, int L, float* out) {
    const XlmrModel& xl = h->xl;
    if (!xl.m.ready) JG_FAIL(h, JG_ERR_STATE, "XLM-RoBERTa weights not finalized (jg_finalize_weights(h, 4))");
    if (B <= 0 || L <= 0 || L > xl.maxpos - 2) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and 0 < L <= %d", xl.maxpos - 2);
    if (audit_mask(h) & AUD_XLMR) {
        if (xl.folded) JG_FAIL(h, JG_ERR_STATE, "the XLM-RoBERTa weights were packed for the implicit-LayerNorm pass: finalize them with audit weights for the fp32 path");
        return xlmr_encode_unfolded(h, A32(), ids, amask, B, L, out);
    }
    if (xl.folded && !h->opts.gemm_glds)      // (plan_gemm would reject every implicit-LayerNorm launch: say why up front)
        JG_FAIL(h, JG_ERR_STATE, "the XLM-RoBERTa weights were packed for the implicit-LayerNorm pass, which needs the LDS-DMA GEMM: set option "
                                 "gemm_glds=0 (or xlmr_fold=0) BEFORE jg_finalize_weights(h, 4)");
    if (xl.folded) return xlmr_encode_folded(h, ids, amask, B, L, out);
    return xlmr_encode_unfolded(h, A16(), ids, amask, B, L, out);
}

}  // namespace engine
