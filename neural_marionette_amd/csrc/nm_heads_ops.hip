// Op-level entry points of the detector heads and losses (nm_op_* of include/nm355.h; unit parity: tests/test_heads_ops_gpu.py).
// Thin wrappers over the launchers of nm_heads.h / nm_heads_bwd.h - the launches the network paths of nm_net.hip make, on tensors the
// caller chooses.  No kernels here.  Scratch comes from the context's workspace arena (as nm_eval_voxel_chamfer takes it), so a call
// must not overlap a network call of the same context.  The backward entries recompute the forward records they need (marginal
// partial sums, Gaussian tables) with the forward launchers, as the training tape would hold them.
#include "nm_ctx.h"
#include "nm_heads.h"
#include "nm_heads_bwd.h"

namespace {

// arena bookkeeping: sum the requests (each rounded up to the arena's 256-byte granule), reserve once, then hand out
struct OpArena {
    nm_ctx* c;
    size_t need = 4096;
    explicit OpArena(nm_ctx* ctx) : c(ctx) {}
    void want(size_t floats) { need += ((floats * sizeof(float) + 255) & ~(size_t)255) + 256; }
    int reserve() {
        int rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice");
        if (rc) return rc;
        if ((rc = nm_ctx_reserve(c, need))) return rc;
        c->ws.release(0);
        return NM_OK;
    }
    float* f(size_t floats) { return c->ws.f(floats); }
};

int zero(float* p, size_t floats, hipStream_t s) { return nm_check_hip(hipMemsetAsync(p, 0, floats * sizeof(float), s), "memset"); }

bool heat_args_ok(const char* who, int B, int T, int K, int Kc, int g) {
    if (B < 1 || T < 1 || K < 1 || K > 32 || Kc < K || Kc % 4 || g < 2 || g > 32) {
        nm_set_error("%s: B=%d T=%d K=%d (row pitch %d) g=%d unsupported", who, B, T, K, Kc, g);
        return false;
    }
    return true;
}

// heat-maps, marginal records, keypoints and means of B clips
int heat_forward(nm_ctx* c, const float* head, const float* clip_head, const float* prop, int B, int T, int K, int Kc, int g, int recurrent,
                 float* heatmaps, float* part, float* keypoints, float* heat_mean) {
    int rc = recurrent ? nm_launch_heatmap_recurrent(head, clip_head, prop, B, T, K, Kc, g, heatmaps, part, c->stream)
                       : nm_launch_heatmap(head, clip_head, prop, B * T, T, K, Kc, g, heatmaps, part, c->stream);
    if (rc) return rc;
    return nm_launch_keypoints(part, B * T, K, g, keypoints, heat_mean, c->stream);
}

float gauss_width(float sigma, int g) { return (float)(2.0 * std::pow((double)sigma / (double)g, 2.0)); }

TensorRef tail_ref(const float* x, const float* scale, const float* shift, float slope, int F, int G, int C) {
    TensorRef t; t.p = x; t.scale = scale; t.shift = shift; t.slope = slope; t.N = F; t.D = t.H = t.W = G; t.C = C;
    return t;
}

}  // namespace

extern "C" {

int nm_op_heatmaps(nm_ctx* c, const float* head, const float* clip_head, const float* prop, int32_t B, int32_t T, int32_t K, int32_t Kc,
                   int32_t g, int32_t recurrent, float* heatmaps, float* keypoints, float* heat_mean) try { NmScope nm_scope_(c);
    if (!c || !head || !clip_head || !prop || !heatmaps || !keypoints || !heat_mean) { nm_set_error("op_heatmaps: null argument"); return NM_ERR_ARG; }
    if (!heat_args_ok("op_heatmaps", B, T, K, Kc, g)) return NM_ERR_ARG;
    const size_t F = (size_t)B * T, pfl = F * K * g * (2 * g + 2);
    OpArena a(c); a.want(pfl);
    int rc = a.reserve();
    if (rc) return rc;
    float* part = a.f(pfl);
    return heat_forward(c, head, clip_head, prop, B, T, K, Kc, g, recurrent, heatmaps, part, keypoints, heat_mean);
} catch (...) { return nm_abi_catch("nm_op_heatmaps"); }

int nm_op_heatmaps_backward(nm_ctx* c, const float* head, const float* clip_head, const float* prop, int32_t B, int32_t T, int32_t K,
                            int32_t Kc, int32_t g, int32_t recurrent, const float* dkp, const float* dloss, float* dhead,
                            float* dclip_head, float* dprop) try { NmScope nm_scope_(c);
    if (!c || !head || !clip_head || !prop || !dkp || !dloss || !dhead || !dclip_head || !dprop) { nm_set_error("op_heatmaps_backward: null argument"); return NM_ERR_ARG; }
    if (!heat_args_ok("op_heatmaps_backward", B, T, K, Kc, g)) return NM_ERR_ARG;
    const size_t F = (size_t)B * T, g3 = (size_t)g * g * g, pfl = F * K * g * (2 * g + 2);
    const size_t wfl = recurrent ? nm_heat_bwd_recurrent_ws_floats(B, T, K, Kc, g) : nm_heat_bwd_ws_floats((int)F, K, g);
    OpArena a(c); a.want(F * K * g3); a.want(pfl); a.want(F * K * 4); a.want(F * K); a.want(wfl);
    if (!recurrent) a.want(F * g3 * Kc);
    int rc = a.reserve();
    if (rc) return rc;
    float* hm = a.f(F * K * g3); float* part = a.f(pfl); float* kp = a.f(F * K * 4); float* mean = a.f(F * K); float* ws = a.f(wfl);
    float* dchead_t = recurrent ? nullptr : a.f(F * g3 * Kc);
    if ((rc = heat_forward(c, head, clip_head, prop, B, T, K, Kc, g, recurrent, hm, part, kp, mean))) return rc;
    if (recurrent) return nm_launch_heat_bwd_recurrent(head, clip_head, prop, part, mean, kp, dkp, dloss, B, T, K, Kc, g, ws, dhead, dclip_head, dprop, c->stream);
    return nm_launch_heat_bwd(head, clip_head, prop, part, mean, kp, dkp, dloss, B, T, K, Kc, g, ws, dhead, dchead_t, dclip_head, dprop, c->stream);
} catch (...) { return nm_abi_catch("nm_op_heatmaps_backward"); }

int nm_op_combined(nm_ctx* c, const float* keypoints, const float* first_feature, const float* sigma_param, int32_t B, int32_t T, int32_t K,
                   int32_t Fd, int32_t g, int32_t Cc, float sigma, int32_t cat, float* table, float* out) try { NmScope nm_scope_(c);
    if (!c || !keypoints || !first_feature || !out) { nm_set_error("op_combined: null argument"); return NM_ERR_ARG; }
    if (B < 1 || T < 1 || K < 1 || K > 32 || Fd < 4 || Fd % 4 || g < 2 || Cc % 4 || Cc < 2 * K + Fd + 3 || cat < 0 || cat > 2) {
        nm_set_error("op_combined: B=%d T=%d K=%d Fd=%d g=%d Cc=%d cat=%d unsupported", B, T, K, Fd, g, Cc, cat); return NM_ERR_ARG;
    }
    const int F = B * T;
    OpArena a(c); a.want((size_t)F * K * 3 * g); a.want(64);
    int rc = a.reserve();
    if (rc) return rc;
    float* tb = table ? table : a.f((size_t)F * K * 3 * g);
    float* widthk = sigma_param ? a.f(64) : nullptr;
    if (widthk && (rc = nm_launch_gauss_width(sigma_param, K, 2.0f * sigma, g, widthk, c->stream))) return rc;
    if ((rc = nm_launch_gauss_table(keypoints, F * K, g, gauss_width(sigma, g), tb, c->stream, widthk, K))) return rc;
    return nm_launch_combined(tb, keypoints, first_feature, 1, F, T, K, Fd, g, Cc, out, c->stream, cat);
} catch (...) { return nm_abi_catch("nm_op_combined"); }

int nm_op_combined_backward(nm_ctx* c, const float* dcomb, int32_t Cd, const float* keypoints, const float* sigma_param, int32_t B,
                            int32_t T, int32_t K, int32_t Fd, int32_t g, float sigma, int32_t cat, float* dfeat, float* dkp,
                            float* dsigma_param) try { NmScope nm_scope_(c);
    if (!c || !dcomb || !keypoints || !dfeat || !dkp || (sigma_param && !dsigma_param)) { nm_set_error("op_combined_backward: null argument"); return NM_ERR_ARG; }
    if (B < 1 || T < 1 || K < 1 || K > 32 || Fd < 4 || Fd % 4 || g < 2 || Cd % 4 || Cd < 2 * K + Fd || cat < 0 || cat > 2) {
        nm_set_error("op_combined_backward: B=%d T=%d K=%d Fd=%d g=%d Cd=%d cat=%d unsupported", B, T, K, Fd, g, Cd, cat); return NM_ERR_ARG;
    }
    const int F = B * T;
    const size_t g3 = (size_t)g * g * g;
    OpArena a(c); a.want((size_t)F * K * 3 * g); a.want(64); a.want((size_t)F * K * 10);
    int rc = a.reserve();
    if (rc) return rc;
    float* tb = a.f((size_t)F * K * 3 * g); float* widthk = sigma_param ? a.f(64) : nullptr; float* ws = a.f((size_t)F * K * 10);
    hipStream_t s = c->stream;
    if (widthk && (rc = nm_launch_gauss_width(sigma_param, K, 2.0f * sigma, g, widthk, s))) return rc;
    if ((rc = nm_launch_gauss_table(keypoints, F * K, g, gauss_width(sigma, g), tb, s, widthk, K))) return rc;
    // (the launcher accumulates into dkp and into frame 0 of every clip of dfeat, as the network's backward walk needs it)
    if ((rc = zero(dfeat, (size_t)F * g3 * Fd, s)) || (rc = zero(dkp, (size_t)F * K * 4, s))) return rc;
    return nm_launch_combined_bwd(dcomb, Cd, tb, keypoints, B, T, K, Fd, g, gauss_width(sigma, g), ws, dfeat, dkp, s, cat, widthk, sigma_param,
                                  2.0f * sigma, dsigma_param);
} catch (...) { return nm_abi_catch("nm_op_combined_backward"); }

int nm_op_decoder_tail(nm_ctx* c, const float* x, const float* scale, const float* shift, float slope, int32_t B, int32_t T, int32_t C,
                       int32_t G, const float* w14, const float* first_frames, int32_t ff_stride_frames, const float* target,
                       const float* keypoints, int32_t K, float* recon, float* frame_sums) try { NmScope nm_scope_(c);
    if (!c || !x || !scale || !shift || !w14 || !first_frames || !recon || (target && !frame_sums)) { nm_set_error("op_decoder_tail: null argument"); return NM_ERR_ARG; }
    if (B < 1 || T < 1 || C < 4 || C % 4 || G < 2 || ff_stride_frames < 0 || (keypoints && (K < 1 || K > 32))) {
        nm_set_error("op_decoder_tail: B=%d T=%d C=%d G=%d K=%d unsupported", B, T, C, G, K); return NM_ERR_ARG;
    }
    const int F = B * T, tb = nm_tail_blocks(G), Kf = 2;
    OpArena a(c); a.want((size_t)F * tb * 3); a.want((size_t)F * Kf); a.want((size_t)B * 5); a.want(16);
    int rc = a.reserve();
    if (rc) return rc;
    float* part = a.f((size_t)F * tb * 3); float* hmean = a.f((size_t)F * Kf); float* clip = a.f((size_t)B * 5); float* losses = a.f(16);
    hipStream_t s = c->stream;
    if ((rc = nm_launch_decoder_tail(tail_ref(x, scale, shift, slope, F, G, C), w14, first_frames, ff_stride_frames, T, target, keypoints, K, G, recon,
                                     target ? part : nullptr, s)) || !target) return rc;
    // the per-frame sums as the network forms them: the first kernel of nm_launch_loss_finalize (its scalar means go to scratch)
    if ((rc = zero(hmean, (size_t)F * Kf, s)) || (rc = zero(clip, (size_t)B * 5, s))) return rc;
    return nm_launch_loss_finalize(part, tb, B, T, Kf, 1, G, hmean, clip, nullptr, 0, 0, frame_sums, losses, s);
} catch (...) { return nm_abi_catch("nm_op_decoder_tail"); }

int nm_op_decoder_tail_backward(nm_ctx* c, const float* x, const float* scale, const float* shift, float slope, int32_t F, int32_t C, int32_t G,
                                const float* w14, const float* target, const float* recon, const float* frame_sums, const float* keypoints,
                                int32_t K, const float* dloss, float* dA, float* dvout, float* dw14, float* dkp) try { NmScope nm_scope_(c);
    if (!c || !x || !scale || !shift || !w14 || !target || !recon || !dloss || !dw14 || (!dA && !dvout) || (dkp && (!keypoints || !frame_sums))) {
        nm_set_error("op_decoder_tail_backward: null argument"); return NM_ERR_ARG;
    }
    if (F < 1 || C < 4 || C % 4 || G < 2 || (dkp && (K < 1 || K > 32))) { nm_set_error("op_decoder_tail_backward: F=%d C=%d G=%d K=%d unsupported", F, C, G, K); return NM_ERR_ARG; }
    const int tb = nm_tail_bwd_blocks(G), cb = nm_chamfer_bwd_blocks(G);
    OpArena a(c); a.want((size_t)F * tb * (C + 1)); a.want(dkp ? (size_t)F * cb * K * 3 : 0);
    int rc = a.reserve();
    if (rc) return rc;
    float* part = a.f((size_t)F * tb * (C + 1)); float* cws = dkp ? a.f((size_t)F * cb * K * 3) : nullptr;
    hipStream_t s = c->stream;
    if ((rc = nm_launch_decoder_tail_bwd(tail_ref(x, scale, shift, slope, F, G, C), w14, target, recon, dloss, G, dvout ? nullptr : dA, part, s, dvout))) return rc;
    if ((rc = nm_launch_sum_rows(part, F * tb, C + 1, dw14, s)) || !dkp) return rc;
    if ((rc = zero(dkp, (size_t)F * K * 4, s))) return rc;
    return nm_launch_chamfer_bwd(target, keypoints, frame_sums, 1, dloss, F, K, G, cws, dkp, s);
} catch (...) { return nm_abi_catch("nm_op_decoder_tail_backward"); }

int nm_op_clip_losses(nm_ctx* c, const float* keypoints, const float* affinity, const float* heat_mean, const float* frame_sums,
                      const float* vol_override, int32_t B, int32_t T, int32_t K, int32_t N, int32_t G, float sep_sigma, int32_t graph_ver,
                      int32_t graph_flags, int32_t use_traj, int32_t vol_fit, float* losses11) try { NmScope nm_scope_(c);
    if (!c || !keypoints || !heat_mean || !frame_sums || !losses11) { nm_set_error("op_clip_losses: null argument"); return NM_ERR_ARG; }
    if (B < 1 || T < 1 || K < 2 || K > 32 || (affinity && N < 1) || G < 2 || (graph_flags & ~15)) {
        nm_set_error("op_clip_losses: B=%d T=%d K=%d N=%d G=%d flags=%d unsupported", B, T, K, N, G, graph_flags); return NM_ERR_ARG;
    }
    OpArena a(c); a.want((size_t)B * 5); a.want((size_t)B * T * 3);
    int rc = a.reserve();
    if (rc) return rc;
    float* clip = a.f((size_t)B * 5); float* fs = a.f((size_t)B * T * 3);
    if ((rc = nm_launch_clip_loss(keypoints, affinity, B, T, K, N, sep_sigma, clip, c->stream, graph_ver))) return rc;
    return nm_launch_loss_finalize(frame_sums, 1, B, T, K, N, G, heat_mean, clip, affinity, vol_fit, use_traj, fs, losses11, c->stream, vol_override, graph_flags);
} catch (...) { return nm_abi_catch("nm_op_clip_losses"); }

int nm_op_clip_losses_backward(nm_ctx* c, const float* keypoints, const float* affinity, const float* dloss, int32_t B, int32_t T, int32_t K,
                               int32_t N, float sep_sigma, int32_t graph_ver, int32_t graph_flags, int32_t use_traj, float* dkp,
                               float* dinfl) try { NmScope nm_scope_(c);
    if (!c || !keypoints || !dloss || !dkp || (affinity && !dinfl)) { nm_set_error("op_clip_losses_backward: null argument"); return NM_ERR_ARG; }
    if (B < 1 || T < 1 || K < 2 || K > 32 || (affinity && N < 1) || (graph_flags & ~15)) {
        nm_set_error("op_clip_losses_backward: B=%d T=%d K=%d N=%d flags=%d unsupported", B, T, K, N, graph_flags); return NM_ERR_ARG;
    }
    int rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice");
    if (rc || (rc = zero(dkp, (size_t)B * T * K * 4, c->stream))) return rc;
    return nm_launch_clip_loss_bwd(keypoints, affinity, dloss, B, T, K, N, sep_sigma, use_traj, dkp, dinfl, c->stream, graph_ver, graph_flags);
} catch (...) { return nm_abi_catch("nm_op_clip_losses_backward"); }

int nm_op_affinity(nm_ctx* c, const float* params, int32_t N, int32_t K, int32_t ver, float* affinity) try { NmScope nm_scope_(c);
    if (!c || !params || !affinity) { nm_set_error("op_affinity: null argument"); return NM_ERR_ARG; }
    if (N < 1 || K < 2 || K > 32 || ver < 0 || ver > 3) { nm_set_error("op_affinity: N=%d K=%d ver=%d unsupported", N, K, ver); return NM_ERR_ARG; }
    int rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice");
    if (rc) return rc;
    return nm_launch_affinity(params, N, K, affinity, c->stream, ver);
} catch (...) { return nm_abi_catch("nm_op_affinity"); }

int nm_op_affinity_backward(nm_ctx* c, const float* params, const float* affinity, const float* dinfl, const float* dloss, int32_t B, int32_t N,
                            int32_t K, int32_t ver, int32_t graph_ver, int32_t graph_flags, float* dparams) try { NmScope nm_scope_(c);
    if (!c || !params || !affinity || !dinfl || !dloss || !dparams) { nm_set_error("op_affinity_backward: null argument"); return NM_ERR_ARG; }
    if (B < 1 || N < 1 || K < 2 || K > 32 || ver < 0 || ver > 3 || graph_ver < 0 || graph_ver > 2 || (size_t)N * K * K * sizeof(float) > 64 * 1024) {
        nm_set_error("op_affinity_backward: B=%d N=%d K=%d ver=%d graph_ver=%d unsupported", B, N, K, ver, graph_ver); return NM_ERR_ARG;
    }
    int rc = nm_check_hip(hipSetDevice(c->cfg.device), "hipSetDevice");
    if (rc) return rc;
    return nm_launch_affinity_bwd(params, affinity, dinfl, dloss, B, N, K, dparams, c->stream, ver, graph_ver, graph_flags);
} catch (...) { return nm_abi_catch("nm_op_affinity_backward"); }

int nm_op_volfit_gauss(nm_ctx* c, const float* vox, const float* keypoints, int32_t B, int32_t T, int32_t K, int32_t G, float sigma,
                       float* vol) try { NmScope nm_scope_(c);
    if (!c || !vox || !keypoints || !vol) { nm_set_error("op_volfit_gauss: null argument"); return NM_ERR_ARG; }
    if (B < 1 || T < 1 || K < 1 || G < 2) { nm_set_error("op_volfit_gauss: B=%d T=%d K=%d G=%d unsupported", B, T, K, G); return NM_ERR_ARG; }
    const size_t wfl = nm_volfit_gauss_ws_floats(B * T, G);
    OpArena a(c); a.want(wfl);
    int rc = a.reserve();
    if (rc) return rc;
    return nm_launch_volfit_gauss(vox, keypoints, B, T, K, G, sigma, a.f(wfl), vol, c->stream);
} catch (...) { return nm_abi_catch("nm_op_volfit_gauss"); }

int nm_op_volfit_gauss_backward(nm_ctx* c, const float* vox, const float* keypoints, const float* dloss, int32_t B, int32_t T, int32_t K,
                                int32_t G, float sigma, float* dkp) try { NmScope nm_scope_(c);
    if (!c || !vox || !keypoints || !dloss || !dkp) { nm_set_error("op_volfit_gauss_backward: null argument"); return NM_ERR_ARG; }
    if (B < 1 || T < 1 || K < 1 || G < 2) { nm_set_error("op_volfit_gauss_backward: B=%d T=%d K=%d G=%d unsupported", B, T, K, G); return NM_ERR_ARG; }
    const size_t wfl = nm_volfit_gauss_bwd_ws_floats(B, T, G);
    OpArena a(c); a.want(wfl);
    int rc = a.reserve();
    if (rc) return rc;
    float* ws = a.f(wfl);
    if ((rc = zero(dkp, (size_t)B * T * K * 4, c->stream))) return rc;
    return nm_launch_volfit_gauss_bwd(vox, keypoints, dloss, B, T, K, G, sigma, ws, dkp, c->stream);
} catch (...) { return nm_abi_catch("nm_op_volfit_gauss_backward"); }

}  // extern "C"
