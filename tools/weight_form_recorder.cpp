// Recorder of tests/golden/weight_form_cases.json: what pack_matrix / gemm() decided about a layer's weights BEFORE the rule moved into
// weight_form.h.  The expressions below are copied from that commit's linear.hip (pack_matrix: the three booleans and the four
// upload(lo) lines; gemm(): the choice of GemmArgs::Wl) with the uploads and the planner stubbed out -- nothing here includes or
// calls weight_form.h, so the table pins the new functions against the old text, not against themselves.
//     g++ -std=c++17 -I include tools/weight_form_recorder.cpp -o /tmp/wfr && /tmp/wfr > tests/golden/weight_form_cases.json
#include <cstdio>
#include <cstdlib>
#include "jegal_hip.h"

enum { LK_CONV = 0, LK_GESTURE = 1, LK_CONTENT = 2, LK_XLMR = 3 };

struct Lin {            // the fields of the old struct Lin that carried the rule; a non-null pointer stands for "uploaded"
    const char* wl = nullptr;
    const char* wl_calib = nullptr;
    bool bc = false, rc = false, bc_pending = false;
};
struct Packed { bool split, bc, rc, lo_uploaded; Lin L; };

static Packed pack_matrix(int mode, int kind, int model_id, bool keep32) {
    static const char lo[] = "lo";
    const bool rcm = mode == JG_PREC_FP16_RC;
    const bool rc = rcm && kind == LK_GESTURE && model_id == 1;
    const bool bc = (mode == JG_PREC_FP16_BC && (kind == LK_GESTURE || kind == LK_XLMR)) || (rcm && kind == LK_XLMR);
    const bool split = kind == LK_CONV ? mode == JG_PREC_FP16_W2_ALL
                                       : (mode == JG_PREC_FP16_W2 || mode == JG_PREC_FP16_W2_ALL || (mode == JG_PREC_FP16_BC && kind == LK_CONTENT) ||
                                          (rcm && !rc && kind != LK_XLMR));
    Packed p = {split, bc, rc, false, Lin()};
    Lin* L = &p.L;
    int uploads = 0;
    L->wl = nullptr;
    if (split) { L->wl = lo; ++uploads; }
    L->bc = bc;
    L->rc = rc;
    L->bc_pending = false;
    if (rc) { L->wl_calib = lo; ++uploads; }
    if (keep32 && !split && !bc && !rc) { L->wl_calib = lo; ++uploads; }
    if (bc) {
        L->wl_calib = lo; ++uploads;
        if (kind == LK_XLMR) { L->wl = L->wl_calib; L->bc_pending = true; }
    }
    if (uploads > 1) { std::fprintf(stderr, "two lo uploads for one layer\n"); std::exit(1); }
    p.lo_uploaded = uploads == 1;
    return p;
}

// gemm(): a.Wl = (h->calib && L.bc) ? L.wl_calib : L.wl;  if (L.rc) { if (can) <per-clip bias> else a.Wl = L.wl_calib; }
static bool gemm_w2(const Lin& L, bool calib, bool can) {
    const char* Wl = (calib && L.bc) ? L.wl_calib : L.wl;
    if (L.rc && !can) Wl = L.wl_calib;
    return Wl != nullptr;
}

int main() {
    std::printf("{\"pack\": [\n");
    int n = 0, two = 0;
    for (int mode = JG_PREC_FP16; mode <= JG_PREC_FP32; ++mode)
        for (int kind = LK_CONV; kind <= LK_XLMR; ++kind)
            for (int model = 1; model <= 3; ++model)
                for (int keep32 = 0; keep32 <= 1; ++keep32) {
                    const Packed p = pack_matrix(mode, kind, model, keep32 != 0);
                    two += p.split + p.bc + p.rc > 1;
                    std::printf("%s{\"precision\": %d, \"kind\": %d, \"model\": %d, \"keep32\": %d, \"split\": %d, \"bc\": %d, \"rc\": %d, \"lo_uploaded\": %d, "
                                "\"wl_after_finalize\": %d, \"bc_pending\": %d}",
                                n++ ? ",\n" : "", mode, kind, model, keep32, p.split, p.bc, p.rc, p.lo_uploaded, p.L.wl != nullptr, p.L.bc_pending);
                }
    if (two) { std::fprintf(stderr, "two forms at once\n"); return 1; }
    // the run-time question per form: a layer as pack_matrix leaves it for that form (one representative (mode, kind, model) each; with and
    // without keep32, which must not matter), `pending` = before apply_bias_corrections has cleared bc_pending (it only ever is set on a bc layer)
    const char* names[4] = {"single", "split", "bias_corrected", "runtime_corrected"};
    const int rep[4][3] = {{JG_PREC_FP16, LK_GESTURE, 1}, {JG_PREC_FP16_W2, LK_GESTURE, 1}, {JG_PREC_FP16_BC, LK_XLMR, 3}, {JG_PREC_FP16_RC, LK_GESTURE, 1}};
    std::printf("\n],\n\"run\": [\n");
    n = 0;
    for (int f = 0; f < 4; ++f)
        for (int pending = 0; pending <= 1; ++pending)
            for (int calib = 0; calib <= 1; ++calib)
                for (int can = 0; can <= 1; ++can) {
                    int w2[2];
                    for (int keep32 = 0; keep32 <= 1; ++keep32) {
                        Lin L = pack_matrix(rep[f][0], rep[f][1], rep[f][2], keep32 != 0).L;
                        if (L.bc && !pending) { L.wl = nullptr; L.bc_pending = false; }      // apply_bias_corrections
                        w2[keep32] = gemm_w2(L, calib != 0, can != 0);
                    }
                    if (w2[0] != w2[1]) { std::fprintf(stderr, "keep32 changes the run-time operand\n"); return 1; }
                    std::printf("%s{\"form\": \"%s\", \"uncalibrated\": %d, \"calibrating\": %d, \"clip_bias\": %d, \"lo\": %d}", n++ ? ",\n" : "", names[f],
                                pending, calib, can, w2[0]);
                }
    std::printf("\n]}\n");
    return 0;
}
