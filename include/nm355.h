/* nm355 — C ABI of the MI355X-native Neural Marionette hot path (libnm355.so).
 *
 * The reference (jinseokbae/neural_marionette) is pure PyTorch: it has no FFI / plugin
 * boundary of its own.  The boundary it exposes for this path is the nn.Module surface
 * of NeuralMarionette / KyptDetector / HSVRNNBVH; this header is the C interface that
 * the drop-in Python shells (neural_marionette_amd/modules.py) bind with ctypes, one
 * entry point per reference method.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous fp32 (or int32 where stated) memory
 *    owned by the caller, in exactly the layout of the reference tensor named in the
 *    comment; the library never keeps a caller pointer past the call's stream-ordered
 *    completion (weights are copied/re-packed into ctx-owned memory by
 *    nm_ctx_set_weights).
 *  - calls are asynchronous on the ctx stream (nm_ctx_set_stream); no hidden device
 *    synchronisation except in create / destroy / set_weights / workspace growth.
 *  - return value: 0 = OK, <0 = error (NM_ERR_*); message via nm_last_error()
 *    (thread-local).  No exceptions or abort() cross this boundary.
 *  - a ctx is bound to one device and one stream and is not thread-safe.
 */
#ifndef NM355_H
#define NM355_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NM_ABI_VERSION 1

#define NM_OK 0
#define NM_ERR_ARG (-1)
#define NM_ERR_HIP (-2)
#define NM_ERR_STATE (-3)
#define NM_ERR_UNSUPPORTED (-4)
#define NM_ERR_RANGE (-5)       /* non-finite conv results (operand beyond the split-fp16 range, or non-finite input) */
#define NM_ERR_INTERNAL (-6)    /* a C++ exception (std::bad_alloc, ...) was caught at the ABI: every entry point is a function-try-block, nothing unwinds into the caller */

typedef struct nm_ctx nm_ctx;

/* Hot-path hyper-parameters (pretrained/aist/opt.pickle of the reference; fields read at
 * model/kypt_detector.py:18-68, model/hsvrnn_bvh.py:14-20). */
typedef struct nm_config {
    int32_t device;          /* HIP device ordinal */
    int32_t grid_size;       /* G: occupancy grid edge (64; multiples of 8 >= 32) */
    int32_t nkeypoints;      /* K (24) */
    int32_t nlatent;         /* Z (128) */
    int32_t nhidden;         /* H (512) */
    int32_t nneighbor;       /* N (2) affinity neighbours */
    float gaussian_sigma;    /* 1.5 */
    float sep_sigma;         /* 0.02 */
    int32_t vol_fit_chamfer; /* vol_fit_type: 1 'chamfer', 0 'none', 2 'gaussian' (kypt_detector_utils.py:154-169, as the reference computes it) */
    int32_t use_graph_traj;  /* graph_traj_weight > 0 */
} nm_config;

typedef struct nm_named_tensor {
    const char* name;        /* state_dict key of the reference module */
    const float* data;       /* device pointer, contiguous fp32, torch layout */
    int64_t numel;
} nm_named_tensor;

int nm_abi_version(void);
const char* nm_last_error(void);
/* Errors: every entry point below is a function-try-block - a C++ exception raised inside the library (std::bad_alloc
 * from a host container, ...) is caught at the boundary and reported as NM_ERR_INTERNAL with its message in nm_last_error(); nothing
 * unwinds into the caller (ctypes / cgo / JNI would abort).  nm_abi_selftest_throw raises such an exception on purpose (kind 0:
 * std::bad_alloc of a real allocation request, 1: std::length_error, 2: a non-std exception) and must return NM_ERR_INTERNAL; it needs
 * no device (tests/test_abi_cpu.py). */
int nm_abi_selftest_throw(int32_t kind);

int nm_ctx_create(nm_ctx** out, const nm_config* cfg);
int nm_ctx_destroy(nm_ctx* ctx);
/* Binds the stream every later call is enqueued on (torch.cuda.current_stream() in the shells).  A ctx works on ONE stream
 * at a time; when the handle changes, the new stream is made to wait (event) for everything the ctx queued on the old one
 * and on its own side stream, so ctx-owned weights / workspaces are never overwritten under a running kernel. */
int nm_ctx_set_stream(nm_ctx* ctx, void* hip_stream);
/* Range / finiteness status.  The default conv arithmetic splits every fp32 operand into two fp16 halves (fp32-equivalent
 * products); an activation of magnitude >= 65520 has no fp16 representation and turns the product into inf / NaN where the
 * reference's fp32 arithmetic (torch CPU ops under kypt_detector.py:81-169) stays finite.  The reference's networks never come
 * near that range (every conv input is a GroupNorm output, an occupancy or a Gaussian map), so the guard is a status word, not a
 * per-launch test: the GroupNorm finalisation of every conv ORs 1 into a ctx-owned device word when the conv's statistics are not
 * finite.  The word is READ AUTOMATICALLY (round 4): every forward-type entry point (nm_detector_forward[_train], nm_forward_fused,
 * nm_vrnn_encode / generate / rollout ...) ends with a 4-byte copy of it into a pinned host slot behind an event, and every entry
 * point begins by looking at the slots whose events have completed - no device synchronisation; a set bit makes THAT call fail
 * with a message naming the call that produced the value and the remedy (nm_set_conv_mode(ctx, 0): exact fp32 MFMA, no range
 * limit): NM_ERR_RANGE for bit 1 (non-finite conv statistics), NM_ERR_STATE for bit 2 (a persistent rollout kernel gave up a bounded
 * wait - never a hang).  nm_ctx_check_nonfinite drains the pending slots synchronously with the same two codes, word cleared; 0
 * otherwise.  The op-level entry point nm_op_conv3d is synchronous about it: it
 * scans its result and re-runs the launch on the fp32 path by itself.  (The Python shells add set_conv_mode('auto').) */
int nm_ctx_check_nonfinite(nm_ctx* ctx);
/* Replaces NeuralMarionette.load_state_dict / .cuda() for the HIP path: copies every
 * tensor and re-packs conv weights into the MFMA layout.  Must be called again after an
 * optimizer step.  All 337 keys of the reference state_dict are required.  Asynchronous on the ctx
 * stream: the source tensors are read in stream order (keep them alive and unmodified until work enqueued
 * before the call's return has drained - PyTorch's stream-ordered allocator guarantees that for tensors of
 * the same stream); a repeated call reuses the ctx-owned buffers and does not synchronise the host. */
int nm_ctx_set_weights(nm_ctx* ctx, const nm_named_tensor* tensors, int32_t count);
/* Bytes of ctx-owned workspace a (B, T) call needs (allocated lazily, grown on demand). */
size_t nm_workspace_bytes(nm_ctx* ctx, int32_t B, int32_t T);
/* Device memory the context owns right now, in bytes: out[0] inference workspace, out[1] training arena (every layer output of the
 * last nm_detector_forward_train + the backward's transients), out[2] the block behind the weight-gradient stream (dY ring, upsample /
 * slot scratch, scale pool), out[3] weights and their packs. */
int nm_ctx_memory(nm_ctx* ctx, size_t out[4]);

/* KyptDetector.forward — model/kypt_detector.py:81-169.
 *  vox        (B,T,1,G,G,G)            in
 *  keypoints  (B,T,K,4)                out  [x1,x2,x3,intensity]
 *  heatmaps   (B,T,K,g,g,g) g=G/4      out
 *  first_feature (B,128,g,g,g)         out
 *  recon      (B,T,1,G,G,G)            out
 *  affinity   (N,K,K,1) or NULL        out  (get_affinity, :171-211, ver 3)
 *  losses11   11 floats                out  order: recon_loss, vol_fit_reg, kypt_const_loss,
 *             separation_loss, sparsity_loss, local_const_loss, time_const_loss,
 *             sparsity_const_loss, intensity_const_loss, graph_traj_loss, graph_vol_loss
 *  affinity_on mirrors KyptDetector.affinity_start (anneal(), :71-78). */
int nm_detector_forward(nm_ctx* ctx, const float* vox, int32_t B, int32_t T, int32_t affinity_on,
                        float* keypoints, float* heatmaps, float* first_feature, float* recon,
                        float* affinity, float* losses11);

/* The part of KyptDetector.forward the learner regime's loss reads (round 5): VoxToKyptNet (model/kypt_detector.py:299-364) and the
 * affinity (:171-211) - keypoints, heat-maps, first-frame feature - WITHOUT KyptToVoxNet (:388-460) and the eleven losses.  The
 * reference's learner-mode step (train.py:376-412 with pretrained_mode 1; model/neural_marionette.py:45-47) runs the whole detector
 * under torch.no_grad() and reads only log['keypoints'] / the affinity from it; the outputs written here are bit-identical to
 * nm_detector_forward's.  Same argument meaning as nm_detector_forward. */
int nm_detector_keypoints(nm_ctx* ctx, const float* vox, int32_t B, int32_t T, int32_t affinity_on,
                          float* keypoints, float* heatmaps, float* first_feature, float* affinity);

/* NeuralMarionette.forward with detector + learner active (model/neural_marionette.py:34-56) in one call:
 * nm_detector_forward followed by nm_vrnn_encode on the detected keypoints, with the VRNN issued on a
 * ctx-owned side stream as soon as the keypoints exist so that it runs beside the decoder (it does not
 * depend on it).  Needs nm_vrnn_set_tree.  Arguments as in the two separate calls. */
int nm_forward_fused(nm_ctx* ctx, const float* vox, int32_t B, int32_t T, int32_t affinity_on, const float* eps,
                     int32_t S, float* keypoints, float* heatmaps, float* first_feature, float* recon,
                     float* affinity, float* losses11, float* kypt_recon, float* R, float* z, float* h,
                     float* scalars2, int32_t* best_idx);

/* KyptDetector.decode_from_dyna — model/kypt_detector.py:213-241.
 *  keypoints (B,Tg,K,4), first_feature (B,128,g,g,g), first_frame (B,1,G,G,G) -> gen (B,Tg,1,G,G,G) */
int nm_decode_from_keypoints(nm_ctx* ctx, const float* keypoints, const float* first_feature,
                             const float* first_frame, int32_t B, int32_t Tg, float* gen);

/* KyptDetector.get_affinity — model/kypt_detector.py:171-210 -> (N,K,K,1); version 3 unless nm_ctx_set_affinity_ver chose another */
int nm_get_affinity(nm_ctx* ctx, float* affinity);
/* options.affinity_ver (model/kypt_detector.py:29,57-68,173-189): 3 (default, every shipped configuration: affinity_params (N,K,K-1)) or
 * 0 / 1 / 2 (affinity_params (N,K,K): row softmax / softplus Gram matrix, zero diagonal, row-normalised / softplus, zero diagonal, row
 * softmax), forward and backward.  Call before nm_ctx_set_weights (a change invalidates loaded weights: the parameter's shape differs).
 * Version 4 (Gumbel noise) is NM_ERR_UNSUPPORTED. */
int nm_ctx_set_affinity_ver(nm_ctx* ctx, int32_t ver);
/* options.gaussian_cat_type (model/kypt_detector.py:396-401): 0 'none' (default, every shipped configuration), 1 'max', 2 'sum' - the K
 * Gaussian channels of the voxel decoder's combined representation all carry the maximum / the sum clipped to [0, 1] over the K maps;
 * forward (nm_detector_forward*, nm_forward_fused, nm_decode_from_keypoints) and backward.  Takes effect at the next call. */
int nm_ctx_set_gaussian_cat(nm_ctx* ctx, int32_t cat);
/* options.fixed_sigma == 0 (model/kypt_detector.py:258-260, 303-306): the state_dict carries `kypt_detector.vox_to_kypt.sigmas` (K), the
 * detector's Gaussian maps take sigma_k = sigmoid(sigmas[k]) * 2 gaussian_sigma (nm_decode_from_keypoints keeps gaussian_sigma, as
 * decode_from_dyna does), and the backward writes that parameter's gradient.  Call before nm_ctx_set_weights.  Not implemented together
 * with vol_fit_type 'gaussian' (NM_ERR_UNSUPPORTED). */
int nm_ctx_set_learnable_sigma(nm_ctx* ctx, int32_t on);
/* options.const_intensity (model/kypt_detector.py:308-347): 3 (default, every shipped configuration) - every frame's heat-map is propagated
 * from the clip's spatio-temporal heat-map - or 2 - frame t >= 1 is propagated from the heat-map of frame t - 1 (:344-345), frame 0 as
 * under 3; forward (nm_detector_forward*, nm_detector_keypoints, nm_forward_fused) and backward (the reverse scan over the clip's frames;
 * the spatio-temporal head hears from frame 0 alone).  The two values share modules, state_dict and weights: takes effect at the next
 * call, no new nm_ctx_set_weights.  0 (no spatio-temporal net: another weight table), 1 (the initial_heatmaps parameter) and 4 are
 * NM_ERR_UNSUPPORTED - the value is judged before the context, so a null context with an unsupported value reports that. */
int nm_ctx_set_const_intensity(nm_ctx* ctx, int32_t v);
/* options.graph_loss_ver, keypoints_detach, using_local_const, using_time_const, using_sparsity_const and keypoints_graph
 * (model/kypt_detector.py:20-30,54-68,112-143; utils/kypt_detector_utils.py:172-265).  ver: 1 (default) or 0 / 2 - the local, time and
 * trajectory terms weighted by the keypoint intensity of the first index (ver 2 also symmetrises the influence, M + M^T); the intensity
 * then receives a gradient.  flags: 0 = every term as the reference's defaults compute it, else an OR of
 *   NM_GRAPH_LOCAL_OFF     local_const_loss is 0 and sends no gradient     (using_local_const = 0)
 *   NM_GRAPH_TIME_OFF      time_const_loss is 0 and sends no gradient      (using_time_const = 0)
 *   NM_GRAPH_SPARSITY_OFF  sparsity_const_loss is 0 and sends no gradient  (using_sparsity_const = 0)
 *   NM_GRAPH_DETACH        the local, time and trajectory terms see the keypoints detached: their gradient reaches the affinity
 *                          parameters only                                (keypoints_detach = 1)
 *   NM_GRAPH_NONE          keypoints_graph 'none': no kypt_detector.affinity_params in the weights, every detector call runs with
 *                          affinity_on = 0 whatever the caller passes, nm_get_affinity fails, the backward writes no affinity gradient.
 * Call before nm_ctx_set_weights (a change of NM_GRAPH_NONE invalidates loaded weights: the table loses / gains a tensor).  Other
 * versions or bits are NM_ERR_UNSUPPORTED. */
#define NM_GRAPH_LOCAL_OFF    1
#define NM_GRAPH_TIME_OFF     2
#define NM_GRAPH_SPARSITY_OFF 4
#define NM_GRAPH_DETACH       8
#define NM_GRAPH_NONE         16
int nm_ctx_set_graph_loss(nm_ctx* ctx, int32_t ver, int32_t flags);

/* Input path on the device: episodic_normalization (zero translation) + voxelize of
 * utils/dataset_utils.py:9-31, evaluated operation by operation in fp64 so that the voxel indices
 * are bit-exact.  points (T,N,3) float64 -> vox (T,1,G,G,G) fp32 {0,1};
 * idx_out (T,N,3) int32 receives the indices (may be NULL).  Does not need weights. */
int nm_voxelize_clip(nm_ctx* ctx, const double* points, int32_t T, int64_t N, double scale, float* vox,
                     int32_t* idx_out);

/* Input path on the device for a batch: crop_sequence + episodic_normalization (with translation and joints) + voxelize of
 * utils/dataset_utils.py:6-31 as the dataset classes call them (dataset/dataset.py:47-88, :123-183), for B crops of sequences that
 * stay in device memory, in the reference's arithmetic for the dtype the data has.
 *   clips_dev (B) descriptors IN DEVICE MEMORY: points (frames,N,3) and joints (frames,J,3) or NULL of the sequence, its number of
 *     frames, the crop's first frame and frame stride, pad != 0: frames past the end repeat the last one (dataset.py:65-68; without
 *     it start + (T-1) sample_rate < frames must hold), and scale / x_trans / z_trans of episodic_normalization.
 *   points_f64 / joints_f64: 0 = float32, 1 = float64, for every clip of the call.  float32 points are normalised in float32
 *     (den = f32(blen + f32(1e-5)), every step rounded) and become float64 at the translation add, as numpy 2 promotes them; float64
 *     points run nm_voxelize_clip's chain with (x_trans, 0, z_trans) added.
 *   vox (B,T,1,G,G,G) fp32 {0,1}.  An index in [-G,-1] wraps to idx + G like numpy's; a row with an index outside [-G,G) or a
 *     non-finite coordinate writes nothing and is counted in bad_rows (B) int32 (the reference raises "Dataset voxelizer error").
 *   joints_out (B,T,J,3): ((j - bmin) scale / den) 2 - 1 without translation, float32 when points and joints both are, else float64;
 *     required when J > 0.  idx_out (B,T,N,3) int32: the indices before the wrap (0 where the
 *     quotient is not finite or beyond int32).  bbox_out (B,6) float64: bmin xyz, bmax xyz of each
 *     clip's crop.  joints_out / idx_out / bbox_out may be NULL.
 * The call copies nothing, synchronises nothing (but for the workspace's first growth) and needs no weights; the descriptors are
 * therefore not readable by it: the caller checks them, the kernels never read past a sequence's last frame, and a clip whose crop
 * does not fit (or whose descriptor is malformed) writes nothing and counts all its T N rows as bad.  NM_ERR_ARG: null
 * clips_dev / vox / bad_rows, B, T, N < 1, J < 0, J > 0 without joints_out; NM_ERR_UNSUPPORTED: B > 65535. */
typedef struct nm_clip_desc {
    const void* points;
    const void* joints;
    int32_t frames, start, sample_rate, pad;
    double scale, x_trans, z_trans;
} nm_clip_desc;
int nm_voxelize_batch(nm_ctx* ctx, const nm_clip_desc* clips_dev, int32_t B, int32_t T, int64_t N, int32_t J, int32_t points_f64,
                      int32_t joints_f64, float* vox, void* joints_out, int32_t* idx_out, double* bbox_out, int32_t* bad_rows);

/* ---- mesh sampling: point sequences from mesh sequences - what the reference's offline preparation computed per frame with
 * trimesh.sample.sample_surface(mesh, 20000) and mesh.face_normals (dataset/dfaust/write_sequence_to_obj.py:20-23, :107-115,
 * dataset/aistpp/prepare_aistpp.py:13-16, :75-83) before it wrote the (frames, 20000, 3) arrays the input path reads ----
 * This is trimesh's algorithm - a face by area, a point in it by two uniforms folded into the triangle - with three changes that make
 * the result independent of the order a parallel machine sums in; it is NOT trimesh's or numpy's random stream and not its bits.  The
 * result is defined by this text alone, in float64, unfused, in exactly this operation order (tests/sample_ref.py restates it in numpy).
 *
 * vertices (T,V,3) float32 (widened exactly) or float64 on the device, triangles (F,3) int32 or int64 on the device, shared by all T
 * frames; count samples per frame.  1 <= F <= 2^21, T, V, count >= 1.
 *   1. face records, per frame and face   a = v1 - v0, b = v2 - v0;  c = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x);
 *      n2 = (c_x c_x + c_y c_y) + c_z c_z;  r = sqrt(n2);  area = 0.5 * r;  normal = float(c / r) per component, (0, 0, 0) where n2 is 0 or
 *      not finite.  A face with a vertex index outside [0, V) reads nothing and has area 0 and normal 0 in every frame; `bad_faces`
 *      counts such rows of `triangles` (once a row, not once a frame).
 *   2. integer weights   amax = the frame's largest finite area, e = the exponent frexp(amax) returns (amax = m 2^e, 0.5 <= m < 1; 0 for
 *      amax = 0);  w_i = (uint64) floor(ldexp(area_i, 32 - e)) < 2^32, 0 for an area that is not finite;  Cum = the inclusive prefix sum
 *      of w over the frame's faces, W = Cum[F - 1] < 2^53.  Integer sums do not depend on their order: any scan gives this table.  A face
 *      whose area is below amax 2^-32 has weight 0.  A frame with W = 0 has no surface: all its points are v0 of face 0 ((0, 0, 0) if that
 *      index lies outside [0, V)), its normals 0, its face indices 0, and `empty_frames` counts it.
 *   3. picks   sample s of frame t has uniforms (u0, u1, u2) in [0, 1):  p = min((uint64) floor(u0 * (double) W), W - 1) (a u0 that is
 *      negative or NaN gives p = 0);  face = the smallest i with Cum[i] > p - a face of weight 0 is never picked;  if u1 + u2 > 1.0
 *      (strictly), u1 = fabs(u1 - 1.0) and u2 = fabs(u2 - 1.0);  point = v0 + (a * u1 + b * u2) per component with the face's a, b of 1.
 *      points (T,count,3) float32 = float(point), normals (T,count,3) float32 = the face's normal, face_index (T,count) int32.
 *   4. uniforms   u (T,count,3) float64 on the device, or with u NULL Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments
 *      9E3779B9 / BB67AE85) under key (seed & 0xffffffff, seed >> 32) at counter (s & 0xffffffff, s >> 32, t, call): call 0's words
 *      (x0, x1, x2, x3) give u0 from (x0, x1) and u1 from (x2, x3), call 1's give u2 from (x0, x1); a pair (hi, lo) becomes
 *      ((hi >> 5) * 67108864.0 + (lo >> 6)) * 2^-53.  Known answers (counter / key -> words): 0 0 0 0 / 0 0 -> 6627e8d5 e169c58d bc57ac4c
 *      9b00dbd8; all ffffffff -> 408f276d 41c83b0e a20bc7c6 6d5451fd; 243f6a88 85a308d3 13198a2e 03707344 / a4093822 299f31d0 ->
 *      d16cfe09 94fdcceb 5001e420 24126ea1.  uniforms_out (T,count,3) float64, if given, receives what was used.
 * nm_sample_surface_workspace - bytes of `scratch` for T frames of F faces (0 for a shape nm_sample_surface refuses): areas, Cum,
 *   face normals, the coarse table (every 64th entry of Cum), chunk sums, the frames' maxima.
 * nm_sample_surface - three passes on the context's stream: face records and the frame maximum (a wave reduction, then an atomic
 *   maximum of the bit pattern of a non-negative double - exact and order-free); weights and their scan (one workgroup per frame up to
 *   16384 faces; above that per 4096-face chunk: chunk sums, their scan, the chunks); the draw (a lane per sample; the frame's coarse
 *   table staged in LDS up to 2048 entries = 131072 faces and searched in global memory above, then the 64-entry segment of Cum).
 *   counters (2) int32 on the device: bad_faces, empty_frames, written by every call.  scratch must be 256-byte aligned.
 * nm_sample_tables - copies areas (T,F) float64 and / or cum (T,F) int64 out of the scratch of a nm_sample_surface call with the same
 *   T and F (either may be NULL).
 * All stream-ordered; nothing synchronises and nothing is allocated.  The only atomics are the integer maximum and the two counters:
 * results are bit-identical from run to run.  Arguments are judged before any launch.  NM_ERR_ARG: null ctx / vertices / triangles /
 * scratch / points / normals / face_index / counters, T, V, F, count < 1, F > 2^21, scratch_bytes below the workspace query, a scratch
 * that is not 256-byte aligned; NM_ERR_UNSUPPORTED: count >= 2^31 - 1024, T * ceil(count / 1024) or T * ceil(F / 256) >= 2^31. */
size_t nm_sample_surface_workspace(int32_t T, int32_t F);
int nm_sample_surface(nm_ctx* ctx, const void* vertices, int32_t vertices_f64, const void* triangles, int32_t triangles_i64, int32_t T,
                      int32_t V, int32_t F, int64_t count, uint64_t seed, const double* u, void* scratch, size_t scratch_bytes,
                      float* points, float* normals, int32_t* face_index, double* uniforms_out, int32_t* counters);
int nm_sample_tables(nm_ctx* ctx, const void* scratch, int32_t T, int32_t F, double* areas, int64_t* cum);

/* ---- body models: posed meshes and joints from SMPL-form pose streams - what the reference's AIST++ preparation computes on the host
 * with smplx before it samples the surface (dataset/aistpp/prepare_aistpp.py:54-62: SMPL(...).forward(global_orient, body_pose, transl,
 * scaling).vertices; :86-89: the joint regressor times the posed vertices, the ground-truth joints of semantic_scores) ----
 * One model form: linear blend skinning with shape and pose blend shapes.  This is NOT smplx's float32 arithmetic, and the order "scale,
 * then translate" of the last step is this library's choice: the AIST++ fork of smplx that takes `scaling` is not available to compare
 * with.  The result is defined by this text alone, in float64, unfused, in exactly this operation order (tests/body_ref.py restates it in
 * numpy).  A dot product of three terms is (a0 b0 + a1 b1) + a2 b2; a "running sum" starts from the stated value and adds one product at a
 * time in ascending index order.
 *
 * MODEL (neural_marionette_amd/body.py, BodyModel), float64 on the device: V vertices, J <= 64 joints, S >= 0 shape coefficients,
 * P = 9 (J - 1).  v_template (V,3); shapedirs (V,3,S); posedirs (P, 3V), row p = 9 (j - 1) + 3 a + b for entry (a, b) of joint j >= 1,
 * column 3 v + c; lbs_weights (V,J); the joint regressor (J,V) as CSR - reg_offsets (J+1) int32, reg_cols (nnz) int32 ascending within a
 * row, reg_vals (nnz) float64; parents (J) int32 ON THE HOST with parents[0] = -1 and 0 <= parents[j] < j.
 *   1. shape, once per (model, betas)   v_shaped[v,c] = the running sum from v_template[v,c] of shapedirs[v,c,s] * betas[s];
 *      J_rest[j,c] = the running sum from 0.0, over row j's CSR entries, of val * v_shaped[col,c].  betas NULL means S = 0.
 *   2. rotations, per (frame, joint)   given as rotations (T,J,3,3) float64, or computed from poses (T,J,3), float32 (widened exactly)
 *      or float64, axis-angle r:  e = r + 1e-8 per component;  angle = sqrt((e_x e_x + e_y e_y) + e_z e_z);  u = r / angle per
 *      component;  s = sin(angle), c = cos(angle);  K = [[0,-u_z,u_y],[u_z,0,-u_x],[-u_y,u_x,0]];  KK_ab = the three-term dot of row a
 *      and column b of K;  R_ab = (I_ab + s * K_ab) + (1 - c) * KK_ab.  A zero vector gives exactly I.  (smplx's batch_rodrigues as it is
 *      remembered; it cannot be compared here.)  This is the one stage with sin, cos and a square root, whose last bits are the math
 *      library's: it is an output, rotations_out (T,J,3,3), so that everything after it can be checked exactly.
 *   3. chain, per frame, j ascending   Gr_0 = R_0, Gt_0 = J_rest_0;  for j > 0 with p = parents[j]: rel = J_rest_j - J_rest_p;
 *      Gr_j = Gr_p R_j (three-term dots);  Gt_j = (Gr_p rel) + Gt_p.  Posed joint Jp_j = Gt_j.  Skinning transform A_j = [Ar_j | At_j]
 *      (3x4): Ar_j = Gr_j, At_j = Gt_j - (Gr_j J_rest_j).
 *   4. vertices, per (frame, vertex)   off_c = the running sum from 0.0, over p ascending, of (R[j,a,b] - I_ab) * posedirs[p, 3v+c];
 *      vp = v_shaped + off;  M (3x4) = the running sum from 0.0, over j ascending, of w[v,j] * A_j entry by entry, terms with
 *      w[v,j] == 0.0 skipped;  x_c = ((M_c0 vp_x + M_c1 vp_y) + M_c2 vp_z) + M_c3;  vertices[t,v,c] = scaling * x_c + transl[t,c]
 *      (transl (T,3) float64; NULL: no addition).  posed_joints[t,j,c] = scaling * Jp_j,c + transl[t,c].
 *   5. regressed joints (prepare_aistpp.py:86-89)   joints[t,j,c] = the running sum from 0.0, over row j's CSR entries, of
 *      val * vertices[t,col,c] - the posed, scaled, translated vertices.
 * A non-finite pose or rotation poisons its own frame only.  A regressor row with an offset pair outside [0, nnz] or a column outside
 * [0, V) reads nothing through the bad entry and is quiet NaN (BodyModel builds no such table).
 * nm_body_shape - step 1: two launches.  reg_cols / reg_vals may be NULL with reg_nnz == 0, shapedirs with S == 0.
 * nm_body_pose - steps 2 to 4: the rotations (a lane per frame and joint; skipped with `rotations`), the chain (a lane per frame and row of the
 *   3x4 transforms walking the J joints, its parents' rows in LDS), the vertices.  The vertex kernel: a lane per vertex, 128 vertices a workgroup, NM_BODY_FRAMES = 8 frames per read of
 *   posedirs, the per-frame sums in registers; the 8 frames' pose features and then their J skinning transforms in LDS, 8 * J * 12 * 8
 *   bytes (18 432 at J = 24, 49 152 at J = 64).  Exactly one of poses and rotations is given; rotations_out is needed with poses.
 *   transforms (T,J,3,4) float64 receives the A_j (scratch the caller owns, and an output).  posedirs may be NULL with J == 1.
 * nm_body_joints - step 5: a lane per (frame, joint, component).
 * All three are stream-ordered, allocate nothing, synchronise nothing and need no weights.  No atomic of any kind is used: results are
 * bit-identical from run to run.  Arguments are judged before any launch.  NM_ERR_ARG: null ctx or a null pointer other than those
 * named optional, T, V, J < 1, J > 64, S < 0, reg_nnz < 0, both or neither of poses / rotations, a parent table that is not topological,
 * a scaling that is zero or not finite; NM_ERR_UNSUPPORTED: T V, T J, 3 V, 3 T J or the vertex kernel's workgroups >= 2^31. */
int nm_body_shape(nm_ctx* ctx, const double* v_template, const double* shapedirs, const double* betas, int32_t V, int32_t S, int32_t J,
                  const int32_t* reg_offsets, const int32_t* reg_cols, const double* reg_vals, int32_t reg_nnz, double* v_shaped,
                  double* J_rest);
int nm_body_pose(nm_ctx* ctx, const void* poses, int32_t poses_f64, const double* rotations, int32_t T, int32_t V, int32_t J,
                 const int32_t* parents_host, const double* v_shaped, const double* J_rest, const double* posedirs,
                 const double* lbs_weights, const double* transl, double scaling, double* rotations_out, double* transforms,
                 double* posed_joints, double* vertices);
int nm_body_joints(nm_ctx* ctx, const double* vertices, int32_t T, int32_t V, int32_t J, const int32_t* reg_offsets,
                   const int32_t* reg_cols, const double* reg_vals, int32_t reg_nnz, double* joints);

/* Device output path: thresholded voxels to ordered point sets - the host lines every consumer of the decoder's voxels starts with
 * (vis_generation.py:137-170, vis_interpolation.py:141-177, vis/visualize.py:58-59, :130-137): binarise, np.where / torch.where per
 * frame, divide into [-1, 1] coordinates, min_z / max_z of the last coordinate over a clip and the per-point (z - min_z) / z_len.
 * vox (B,T,1,G,G,G) fp32 on the device, contiguous, any 4-byte alignment; G need not be the context's grid_size.  F = B T frames.
 * Points come in np.where's order: frame after frame, inside a frame by rising flat position (i G + j) G + k.
 *
 * nm_occupied_count - which voxels are occupied, how many per frame, and each clip's range along the last axis.
 *   mode NM_OCC_THRESHOLD: occupied iff NOT (v < thr) - what `x[x < thr] = 0; x[x >= thr] = 1` leaves non-zero, so a NaN is
 *   occupied; NM_OCC_NONZERO: occupied iff v != 0 (torch.where(x); thr is ignored; NaN occupied, -0.0 empty).
 *   bits: F * ceil(G^3 / 64) 64-bit words, caller-owned - bit j of word w of a frame is its flat voxel 64 w + j, pad bits are zero
 *   (as bytes: np.packbits(occ, bitorder='little') per frame, padded to 8-byte multiples).  offsets (F + 1) int64: the first row of
 *   each frame, offsets[F] = the number of points.  z_idx_range (B,2) int32: the smallest / largest last-axis index over the clip's
 *   T frames, (INT32_MAX, -1) for a clip without a point.  z_range (B,2): the same as coordinates in the arithmetic coord_f64
 *   selects (below), (1e4, -1) - the scripts' initial values - for a clip without a point.
 * nm_occupied_write - the points, from the three arrays nm_occupied_count wrote (the voxels are not read again).
 *   coord_f64 != 0: numpy's arithmetic, double(i) / ((G - 1) / 2.0) - 1.0, coords (N,3) float64; 0: torch's,
 *   float(i) / float((G - 1) / 2.0) - 1.0f, coords (N,3) float32 (the two are not roundings of each other).  idx (N,3) int32: i, j, k.
 *   depth (N) float64, coord_f64 != 0 only: (c_k - min_z) / (max_z - min_z) with the point's own clip's z_range; NaN where the range is
 *   zero, as numpy gives.  Any of idx / coords / depth may be NULL.  Only rows below `capacity` are written (size the buffers by
 *   offsets[F], or by a bound of the caller's - offsets always holds the true counts).
 * Both are stream-ordered, synchronise nothing (but for the workspace's first growth), need no weights and give bit-identical
 * results from run to run (no atomics).  NM_ERR_ARG: null ctx / vox / bits / offsets / z_idx_range / z_range, B, T < 1, G < 2, an
 * unknown mode, depth with coord_f64 = 0, capacity < 0; NM_ERR_UNSUPPORTED: B T G^3 >= 2^31. */
#define NM_OCC_THRESHOLD 0
#define NM_OCC_NONZERO   1
int nm_occupied_count(nm_ctx* ctx, const float* vox, int32_t B, int32_t T, int32_t G, int32_t mode, float thr, int32_t coord_f64,
                      uint64_t* bits, int64_t* offsets, int32_t* z_idx_range, void* z_range);
int nm_occupied_write(nm_ctx* ctx, const uint64_t* bits, const int64_t* offsets, const int32_t* z_idx_range, int32_t B, int32_t T,
                      int32_t G, int32_t coord_f64, int64_t capacity, int32_t* idx, void* coords, double* depth);

/* ---- surface path: normals, plate frames and shading of those points (vis_generation.py:157-171, vis_interpolation.py:160-177: open3d's
 * estimate_normals + orient_normals_consistent_tangent_plane, then the scripts' per-point loop with drawPlate :27-44) ----
 * nm_occupied_surface takes the three arrays nm_occupied_count wrote (the voxels are not read again) and writes one row per point, in
 * nm_occupied_write's order; only rows below `capacity` are written, any output may be NULL.  For the point p = (i, j, k) of frame f:
 *   neighbourhood  the occupied voxels q of the same frame, inside the grid, with |q - p|^2 <= radius2 (1 .. 16), p itself included.
 *   moments (N,10) int32, exact: with d = q - p: n, S = sum d (x, y, z), Q = sum d d^T (xx, xy, xz, yy, yz, zz).
 *   normals (N,3) float64: C = n Q - S S^T is an exact integer matrix; the unit eigenvector of its smallest eigenvalue, solved in float64.
 *     n < 3: (0, 0, 1), as open3d gives a neighbourhood without extent.  spread (N,3) float64: C's eigenvalues, ascending.
 *   orientation  NM_SURF_OUTWARD: n . o >= 0 for o = -S, away from the local mass; if S = 0 as integers, o = N_f p - sum_f q, away from
 *     the frame's centroid; if that is 0 too, o = (1, 1, 1); a dot product of exactly 0.0 leaves the solver's sign.  NM_SURF_TOWARDS:
 *     n is flipped when n . (orient_point[b] - coords(p)) < 0, orient_point (B,3) float64 on the device - open3d's
 *     orient_normals_towards_camera_location - with coords as nm_occupied_write's float64 arithmetic gives them.
 *   plates (N,3,4) float64: rows [R | centre] of drawPlate's transform for centre = coords(p) and the oriented normal:
 *     line2 = n / (|n| + 1e-6), c = line2_z + 1e-8, R = I + K + K^2 / (1 + c), and R = diag(-1, 1, -1) where |c + 1| < 1e-4.
 *   colors (N,3) float64: base[f] * (depth * shade_a + shade_b) (+ add[f] when add is not NULL), base / add (F,3) float64 on the
 *     device, depth as nm_occupied_write defines it (NaN where the clip's range is zero), in numpy's operation order, unfused.
 * These are NOT open3d's normals: on a voxel lattice its 30-nearest-neighbour set is cut inside a shell of equidistant points by the
 * tie-breaking of its k-d tree, so the neighbourhood here is the lattice ball above and the result is defined by this text alone.
 * Stream-ordered, synchronises nothing (but for the workspace's first growth), needs no weights, bit-identical from run to run (no
 * atomics).  NM_ERR_ARG: radius2 outside 1 .. 16 (judged first, before the context), null ctx / bits / offsets / z_idx_range, an unknown
 * orient, NM_SURF_TOWARDS with normals or plates but no orient_point (moments, spread and colors take no orientation: with only those
 * outputs orient_point is never read and may be NULL), colors without base, B, T < 1, G < 2, capacity < 0; NM_ERR_UNSUPPORTED:
 * B T G^3 >= 2^31. */
#define NM_SURF_OUTWARD 0
#define NM_SURF_TOWARDS 1
int nm_occupied_surface(nm_ctx* ctx, const uint64_t* bits, const int64_t* offsets, const int32_t* z_idx_range, int32_t B, int32_t T,
                        int32_t G, int32_t radius2, int32_t orient, const double* orient_point, const double* base, const double* add,
                        double shade_a, double shade_b, int64_t capacity, int32_t* moments, double* normals, double* spread,
                        double* plates, double* colors);

/* ---- render path: those plates drawn as flat discs through a pinhole camera (vis_generation.py:171-190, vis_interpolation.py:177-185:
 * a cylinder mesh per plate into open3d's off-screen visualiser, capture_screen_float_buffer, (img * 255).astype(uint8)) ----
 * This is NOT open3d's image: its lighting, MSAA and GL rasterisation rules are neither available nor reproducible.  The result is
 * defined by this text alone, in float64, unfused, in exactly this operation order (tests/render_ref.py restates it in numpy).
 *   scene    N plates in F frames, frame f owns the rows offsets[f] .. offsets[f+1] of plates (N,3,4) - nm_occupied_surface's arrays;
 *     only rows below `rows` are read, the others are not drawn.  Plate i is the disc with centre c = plates[i,:,3], axis
 *     a = plates[i,:,2] (the third column of drawPlate's R, the image of (0,0,1)) and radius `radius` (the scripts' cylinder: 0.03): the
 *     cylinder's cap at the centre.  Its 0.01 side wall is not drawn; both faces are visible.
 *   camera   open3d's PinholeCameraParameters as nm_camera, a HOST struct: extrinsic = the world -> camera matrix E, row-major (E[r][c] =
 *     extrinsic[4 r + c]; open3d's JSON lists it column-major), fx, fy, cx, cy, width, height and a near plane (open3d has none; 1e-3 is
 *     the shells' default).  Camera axes: x right, y down, z forward.  Pixel (px, py), row 0 at the top as capture_screen_float_buffer
 *     gives it, looks along d = ((px - cx) / fx, (py - cy) / fy, 1) from the origin - open3d's convention, the principal point
 *     cx = width / 2 - 0.5 is the centre of the middle pixel.
 *   per plate, once   c'_r = ((E[r,0] c_x + E[r,1] c_y) + E[r,2] c_z) + E[r,3];  a'_r = (E[r,0] a_x + E[r,1] a_y) + E[r,2] a_z;
 *     q = (a'_x c'_x + a'_y c'_y) + a'_z c'_z.  A plate with c'_z - radius < near, or with a non-finite component of c' or a', is not
 *     drawn at all.
 *   per pixel and plate   den = (a'_x dx + a'_y dy) + a'_z, den == 0 is a miss;  s = q / den, a miss unless s >= near;
 *     h = (s dx - c'_x, s dy - c'_y, s - c'_z), m = (h_x^2 + h_y^2) + h_z^2;  a hit iff m <= radius * radius.
 *   winner   the hit with the smallest s; among equal s the lowest row index.
 *   outputs, any of which may be NULL:  index (F,H,W) int32, the winner's row or -1 for background;  depth (F,H,W) float64, the winner's
 *     s or +inf;  image (F,H,W,3) uint8:  v = colors[i,ch] * (light_a + light_b * |den| / sqrt((dx^2 + dy^2) + 1)) with the winner's
 *     den, NaN -> 0, clamped to [0, 1], stored as uint8(v * 255.0), truncated; background pixels take `background` (3 doubles on the
 *     HOST, NULL = white) through the same NaN / clamp / truncation.  light (1, 0) gives colors as they are - the scripts' depth shading
 *     is in nm_occupied_surface's colors already; light_b weighs the cosine between the plate's axis and the ray (for a unit axis).
 * nm_render_bin - per plate c', a', q and the frame into xf (rows,8) float64 and into rect (rows,4) int32 a pixel rectangle x0, x1, y0,
 *   y1 that contains every pixel the plate can hit (x0 > x1: not drawn); then the number of plates per (frame, 16 x 16-pixel tile),
 *   scanned: tile_offsets (F TY TX + 1) int64, TX = ceil(width / 16), TY = ceil(height / 16), tile (f, ty, tx) at (f TY + ty) TX + tx.
 *   Its last entry is the number of list entries nm_render_draw needs - always the true number.
 * nm_render_draw - fills list (capacity) int32 with the tiles' rows from xf / rect / tile_offsets as nm_render_bin wrote them for the same
 *   arguments, then draws: a workgroup per tile, a thread per pixel.  Only list entries below `capacity` are written or read: with a
 *   capacity below tile_offsets' last entry nothing faults and nothing is written out of bounds, but the image is INCOMPLETE (which
 *   plates the cut tiles lose is not defined); compare the two numbers.  colors (rows,3) float64 may be NULL without image.
 * Integer atomics order the tile lists; the per-pixel minimum over (s, row) does not depend on that order, and no atomic touches an
 * output: results are bit-identical from run to run.  Both are stream-ordered, synchronise nothing (but for the workspace's first
 * growth) and need no weights.  NM_ERR_ARG: null ctx / offsets / camera / tile_offsets, null plates / xf / rect with rows > 0, null list
 * with capacity > 0, image with rows > 0 but no colors, F, width, height < 1, rows < 0, radius not a finite number > 0, capacity < 0, a
 * non-finite camera number, fx or fy of 0, near <= 0; NM_ERR_UNSUPPORTED: F height width >= 2^31, rows >= 2^31. */
typedef struct {
    double extrinsic[16];
    double fx, fy, cx, cy, near;
    int32_t width, height;
} nm_camera;
int nm_render_bin(nm_ctx* ctx, const double* plates, const int64_t* offsets, int32_t F, int64_t rows, const nm_camera* camera, double radius,
                  double* xf, int32_t* rect, int64_t* tile_offsets);
int nm_render_draw(nm_ctx* ctx, const double* xf, const int32_t* rect, const int64_t* offsets, const int64_t* tile_offsets,
                   const double* colors, int32_t F, int64_t rows, const nm_camera* camera, double radius, double light_a, double light_b,
                   const double* background, int64_t capacity, int32_t* list, int32_t* index, double* depth, uint8_t* image);

/* ---- render path for the retargeting demo: the posed triangle mesh, the skeleton, and the skeleton over the mesh (vis_retarget.py:400-557:
 * a TriangleMesh per frame, drawSphere per visible joint, drawCone1 + drawCone2 per bone, img[cone_img.sum(-1) != 3] = cone_img[...]) ----
 * As for the plates this is NOT open3d's image; the result is defined by this text alone, in float64, unfused, in exactly this operation
 * order (tests/mesh_ref.py restates it in numpy).  The camera, the pixel rays d = (dx, dy, 1) = ((px - cx) / fx, (py - cy) / fy, 1), the depth
 * s along the camera's z, the conversion v -> uint8 (NaN -> 0, clamped to [0, 1], uint8(v * 255.0) truncated), `background` (3 doubles on
 * the HOST, NULL = white) and the point formula p'_r = ((E[r,0] p_x + E[r,1] p_y) + E[r,2] p_z) + E[r,3] are the plate contract's above: a
 * mesh depth, a skeleton depth and a plate depth at the same pixel are comparable.  Below A = (dx^2 + dy^2) + 1, a dot product of
 * 3-vectors is u . v = (u_x v_x + u_y v_y) + u_z v_z, one with the ray is u . d = (u_x dx + u_y dy) + u_z, and the headlight of a normal
 * n with den = n . d is  shade = light_a + light_b * |den| / (sqrt(n . n) * sqrt(A)) - light (1, 0) gives the colours as they are.
 *
 * MESH.  vertices (F,V,3) float64 (sample_retarget's points), triangles (M,3) int32 shared by all frames, colours either vertex_colors
 * (V,3) float64 on the device, shared by all frames, or with vertex_colors NULL the uniform `color` (3 doubles on the HOST, NULL = 0.7
 * grey).  All arithmetic is in camera space.
 *   per triangle and frame, once   p'_0, p'_1, p'_2;  e1 = p'_1 - p'_0, e2 = p'_2 - p'_0;  n = e1 x e2 = (e1_y e2_z - e1_z e2_y,
 *     e1_z e2_x - e1_x e2_z, e1_x e2_y - e1_y e2_x);  q = n . p'_0;  X_k = p'_kx / p'_kz, Y_k = p'_ky / p'_kz, iz_k = 1.0 / p'_kz.
 *     A triangle is not drawn at all if one of its indices lies outside [0, V) (judged on the device, nothing is read through it), if a
 *     component of a p'_k, of n or q is not finite, if any vertex has p'_kz < near - the WHOLE triangle is culled, there is NO clipping
 *     against the near plane - or if n is the zero vector.
 *   per pixel: coverage   a_k = X_k - dx, b_k = Y_k - dy;  w0 = a_1 * b_2 - b_1 * a_2, w1 = a_2 * b_0 - b_2 * a_0, w2 = a_0 * b_1 - b_0 * a_1.
 *     (Swapping an edge's two vertices negates its w exactly in IEEE arithmetic, so two triangles that share an edge never leave a crack
 *     along it.)  Covered iff w0, w1, w2 are all >= 0 or all <= 0 - both faces are visible - and (w0 + w1) + w2 != 0, and the pixel lies
 *     in the triangle's rectangle: floor(min_k u_k - 1.0) <= px <= ceil(max_k u_k + 1.0) with u_k = cx + fx * X_k, and the same for py with
 *     v_k = cy + fy * Y_k.  (For a triangle with area the rectangle excludes nothing the edge functions cover; for one seen edge-on,
 *     whose edge functions are rounding noise all along its line, it bounds what that noise can reach.)
 *   per pixel: depth   den = n . d, den == 0 is a miss;  s = q / den, a miss unless s >= near.
 *   winner   the smallest s; among equal s the lowest triangle row (a pixel on a shared edge belongs to both triangles).
 *   colour   l_k = w_k * iz_k, L = (l_0 + l_1) + l_2, colour_ch = ((l_0 c_0,ch + l_1 c_1,ch) + l_2 c_2,ch) / L from the winner's three vertex
 *     colours (perspective-correct), or the uniform colour;  v_ch = colour_ch * shade with the flat face normal n and the winner's den.
 *   outputs, any of which may be NULL:  index (F,H,W) int32, the winner's triangle row or -1;  depth (F,H,W) float64, its s or +inf;
 *     image (F,H,W,3) uint8.
 * nm_mesh_bin - per (frame, triangle), record f M + m: rec (F M,16) float64 = X_0 Y_0 X_1 Y_1 X_2 Y_2, n, q, iz_0 iz_1 iz_2, three zeros
 *   (all zeros for a triangle that is not drawn), and into rect (F M,4) int32 a pixel rectangle x0, x1, y0, y1 that contains every pixel
 *   the triangle can cover (x0 > x1: not drawn); then the number of records per (frame, 16 x 16-pixel tile), scanned: tile_offsets
 *   (F TY TX + 1) int64 laid out as nm_render_bin's, its last entry the number of list entries nm_mesh_draw needs - always the true number.
 * nm_mesh_draw - fills list (capacity) int32 with the tiles' records from rect / tile_offsets as nm_mesh_bin wrote them for the same
 *   arguments, then draws: a workgroup per tile, a thread per pixel, the tile's records through LDS 128 at a time, the vertex colours
 *   fetched for the winner only.  `capacity` works as nm_render_draw's: below tile_offsets' last entry nothing faults and nothing is
 *   written out of bounds, but the image is INCOMPLETE.  triangles may be NULL without vertex_colors or image.  With index, depth and
 *   image all NULL the call does nothing: the list is not filled either.
 *
 * SKELETON.  keypoints (F,K,4) float32 on the device (x, y, z, intensity; converted to float64 first), parents (K) int32 on the device,
 * K <= 32.  Joint k is VISIBLE iff clip(intensity_k, 0, 1) >= threshold (vis_retarget.py:516-522; the script's VIS_THRESHOLD is 0.2; a NaN
 * is not) and its p'_k is finite.
 *   sphere k (primitive k)   for a visible joint with p'_kz - radius >= near (the plates' rule), centre c = p'_k:  C = c . c - radius * radius.
 *     per pixel  B = c . d, D = B * B - A * C;  a hit iff D >= 0 and B > 0;  s = C / (B + sqrt(D)) (the near root, free of cancellation);
 *     normal h = (s dx - c_x, s dy - c_y, s - c_z).
 *   bone of joint k (primitive K + k)   iff k and p = parents[k] are visible, 0 <= p < K, p != k, b = p'_k - p'_p has b . b > 0 (finite), and
 *     both ends have p'_z - bone_radius >= near (no clipping).  It is the script's double cone: two finite nappes that share the base
 *     circle of radius bone_radius about g = p'_p + 0.2 * b (componentwise), perpendicular to the bone, with their apexes at the parent
 *     and at the child.  The shared base disc is interior and is not drawn.  drawCone2's 0.195 margin and the + 1e-6 of the heights are
 *     NOT reproduced: the nappes meet exactly.
 *   nappe with apex a (first p'_p, then p'_k)   v = g - a, vv = v . v, kappa = (vv + bone_radius * bone_radius) / (vv * vv), av = a . v,
 *     aa = a . a (a bone with vv == 0 or a non-finite kappa on either side is not drawn).  Its surface is kappa ((X - a) . v)^2 = |X - a|^2
 *     with 0 <= (X - a) . v <= vv.  per pixel  dv = v . d, da = a . d, kd = kappa * dv;  c2 = kd * dv - A, c1 = kd * av - da,
 *     c0 = (kappa * av) * av - aa: the ray meets the full cone where c2 s^2 - 2 c1 s + c0 = 0.  c2 == 0 is a miss;  D = c1 * c1 - c2 * c0, a
 *     miss unless D >= 0.  The root (c1 + g sqrt(D)) / c2, g = +-1, has the axis parameter (P + g dv sqrt(D)) / c2 with P = c1 * dv - av * c2;
 *     it is ON the nappe iff that lies in [0, vv], which is decided without a square root: for c2 > 0 iff ge0(P, g dv) and
 *     ge0(-P2, -g dv), for c2 < 0 iff ge0(-P, -g dv) and ge0(P2, g dv), where P2 = P - vv * c2 and ge0(p, q), "p + q sqrt(D) >= 0", is: for
 *     q >= 0, p >= 0 or (q * q) * D >= p * p; for q < 0, p >= 0 and p * p >= (q * q) * D.  The hit is the nearer root (g = -1 for c2 > 0, +1 for
 *     c2 < 0) if it is on the nappe, else the other root if that one is, else a miss.  (A ray steeper than the cone meets the nappe at
 *     its far root only, the near one lying on the mirror nappe behind the apex.)  Only now  r = sqrt(D), qq = c1 + r for c1 >= 0 and
 *     c1 - r otherwise, qq == 0 a miss;  the root with g = +1 is qq / c2 for c1 >= 0 and c0 / qq otherwise, the root with g = -1 the other
 *     of the two.  Normal h = (s d - a) - (kappa * (s * dv - av)) v.  A bone's s is the smaller of its nappes' (the parent's on a tie).
 *     A skeleton hit is not compared with near again: what is drawn lies wholly beyond it.
 *   winner   the smallest s, then the lowest primitive number; index stores that number, depth s.
 *   image   v_ch = colour_ch * shade with the normal h at the hit; a sphere takes joint_colors[k] ((K,3) float64 on the device) or with
 *     joint_colors NULL `joint_color`, a bone `bone_color` (3 doubles each on the HOST; NULL = the script's (0.7, 0.1, 0) and (0, 0.6, 0.1)).
 *     With overlay != 0 image is in-out: pixels the skeleton does not cover are left as they are - the script's paste (:463, :550) without
 *     its accident of treating white skeleton pixels as background; otherwise they take `background`.
 * nm_skeleton_draw - one launch, a workgroup per tile, a thread per pixel; the frame's joints and bones are transformed into LDS by the
 *   workgroup, at most 32 spheres and 31 bones, no binning.
 *
 * Integer atomics order the mesh's tile lists only; no atomic touches an output: results are bit-identical from run to run.  All three are
 * stream-ordered, synchronise nothing (but for the workspace's first growth) and need no weights.  Arguments are judged before any launch.
 * NM_ERR_ARG: null ctx / camera, null tile_offsets, null vertices / triangles / rec / rect with M > 0, null list with capacity > 0,
 * vertex_colors with an image but no triangles, null keypoints / parents, F, V, K, width, height < 1, M < 0, K > 32, radius or bone_radius
 * not a finite number > 0, capacity < 0, a non-finite camera number, fx or fy of 0, near <= 0; NM_ERR_UNSUPPORTED: F height width >= 2^31,
 * F M >= 2^31. */
int nm_mesh_bin(nm_ctx* ctx, const double* vertices, const int32_t* triangles, int32_t F, int32_t V, int64_t M, const nm_camera* camera,
                double* rec, int32_t* rect, int64_t* tile_offsets);
int nm_mesh_draw(nm_ctx* ctx, const double* rec, const int32_t* rect, const int64_t* tile_offsets, const int32_t* triangles,
                 const double* vertex_colors, const double* color, int32_t F, int32_t V, int64_t M, const nm_camera* camera, double light_a,
                 double light_b, const double* background, int64_t capacity, int32_t* list, int32_t* index, double* depth, uint8_t* image);
int nm_skeleton_draw(nm_ctx* ctx, const float* keypoints, const int32_t* parents, int32_t F, int32_t K, const nm_camera* camera,
                     double threshold, double radius, double bone_radius, const double* joint_colors, const double* joint_color,
                     const double* bone_color, double light_a, double light_b, const double* background, int32_t overlay, int32_t* index,
                     double* depth, uint8_t* image);

/* ---- Loop subdivision and smooth vertex normals of posed meshes (vis_retarget.py:416-423, :497-512: temp_mesh.subdivide_loop(
 * arg.subdivide_iter) and compute_vertex_normals() on every frame, in open3d on the host), and the mesh shaded with those normals ----
 * This is NOT open3d's result: open3d numbers the new vertices in traversal order and sums unit face normals unweighted.  The result is
 * defined by this text alone, in float64, unfused, in exactly this operation order (tests/subdiv_ref.py restates it).  The topology is a
 * PLAN of index tables, built once per mesh on the host (neural_marionette_amd/subdivide.py, LoopPlan.build); the device applies them
 * per frame.  All tables are int32 on the device but w, which is float64; they are shared by all frames.
 *
 * PLAN, one level: V vertices, triangles (M,3) with every index in [0, V), no triangle with a repeated index, no undirected edge in more
 * than two triangles (LoopPlan.build refuses the rest).
 *   edges      the E undirected edges {a < b}, sorted by (a, b); edge e creates vertex V + e.  edge (E,4) = a, b, c, d: c and d are the
 *     vertices opposite the edge in its triangles, in ascending triangle-row order; d = -1 marks a boundary edge (one triangle).
 *   children   parent row m = (i, j, k) with the edge vertices p = ev(i,j), q = ev(j,k), r = ev(k,i) gives the rows 4m .. 4m+3 =
 *     (i,p,r) (p,j,q) (r,q,k) (p,q,r): the winding is kept.  The next level is built from these rows over V + E vertices.
 *   rings      ring_offsets (V+1), ring (ring_len), w (V,2) = (w_self, w_ring).  A vertex with no boundary edge and n >= 1 edges: its n
 *     neighbours in ascending order, w_ring = beta_n = (0.625 - (0.375 + 0.25 cos(2 pi / n))^2) / n (C's cos, float64, on the host),
 *     w_self = 1 - n beta_n.  A vertex with exactly two boundary edges: those two neighbours in ascending order, (0.75, 0.125).  Any
 *     other vertex (unreferenced, or a bow-tie with another number of boundary edges): an empty list and (1, 0) - it stays where it is.
 *     The weights are plan data; the device only multiplies by them.
 *   finest level only   triangles (M,3), and the vertex -> triangle index face_offsets (V+1), faces (3 M): each vertex's triangle rows,
 *     ascending.
 * nm_subdiv_apply - one level for T frames: in (T,V,3) float64 -> out (T,V+E,3) float64 (posed points, or any three values per vertex
 *   such as colours), per frame and component x:
 *     row v < V (old vertex)     s = 0.0; for j = ring_offsets[v] .. ring_offsets[v+1] - 1 in that order: s = s + x[ring[j]];
 *                                out = w_self * x[v] + w_ring * s
 *     row V + e, d >= 0          out = 0.375 * (x[a] + x[b]) + 0.125 * (x[c] + x[d])
 *     row V + e, d == -1         out = 0.5 * (x[a] + x[b])
 *   The tables are judged on the device, nothing is read through a bad entry: a, b, c or a ring entry outside [0, V), d outside [0, V)
 *   other than -1, ring_offsets[v] < 0, ring_offsets[v+1] > ring_len or ring_offsets[v] > ring_offsets[v+1].  A row with a bad entry is
 *   quiet NaN in every frame and component; bad_rows (1) int32 on the device receives the number of such rows (each once, whatever T) -
 *   every call writes it, 0 for a plan of LoopPlan.build.  edge may be NULL with E == 0, ring with ring_len == 0.
 * nm_vertex_normals - vertices (F,V,3) float64 -> normals (F,V,3) float64, per frame and vertex:  acc = (0, 0, 0);  for each triangle
 *   row m of faces[face_offsets[v] .. face_offsets[v+1]) in that order, with its vertices p0 p1 p2 in the row's order (whichever of
 *   them v is): e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2 by the MESH formula above, acc = acc + c componentwise;
 *   r = sqrt((acc_x acc_x + acc_y acc_y) + acc_z acc_z);  normal = acc / r componentwise, or (0, 0, 0) where r is 0 or not finite.  The
 *   cross product has twice the triangle's area for its length: the normal is AREA-WEIGHTED on purpose (open3d's is not), so a sliver
 *   does not turn the normal of a vertex it touches.  Bad entries - an offset pair as above with 3 M for ring_len, a faces entry outside
 *   [0, M), a vertex of such a triangle outside [0, V) - make the vertex's row quiet NaN in every frame and count once in bad_rows.
 *   triangles and faces may be NULL with M == 0 (every normal is zero).
 * nm_mesh_shade - a deferred pass over index (F,H,W) as nm_mesh_draw wrote it from the same rec (nm_mesh_bin's, F M rows of 16 with iz at
 *   entries 10 .. 12), camera, triangles and vertices: image (F,H,W,3) uint8 is written again with SMOOTH shading from normals (F,V,3)
 *   float64 (nm_vertex_normals' rows, world space).  For a pixel with winner m >= 0:  a_k, b_k, w_k from the record exactly as MESH
 *   coverage does;  l_k = w_k * iz_k, L = (l_0 + l_1) + l_2;  each vertex normal in camera space n'_r = (E[r,0] n_x + E[r,1] n_y) + E[r,2] n_z;
 *   h_r = ((l_0 n'_0,r + l_1 n'_1,r) + l_2 n'_2,r) / L;  shade = light_a + light_b * |h . d| / (sqrt(h . h) * sqrt(A)); where h . h is 0 or
 *   not finite the MESH shade of the record's flat n.  Colour (vertex_colors (V,3) or `color`) and the uint8 conversion as in the draw;
 *   pixels with index -1 take `background` - as do, judged on the device, pixels whose index lies outside [0, M) or whose triangle has a
 *   vertex outside [0, V).  nm_mesh_draw and its results are untouched: draw with image NULL, then shade.
 * All three are stream-ordered, synchronise nothing (but for the workspace's first growth: nm_subdiv_apply and nm_vertex_normals keep one
 * int32 per workgroup there) and need no weights.  No atomic of any kind is used: every output row is written by the one lane that owns it
 * and bad_rows by a single-workgroup sum, so results are bit-identical from run to run.  Arguments are judged before any launch.
 * NM_ERR_ARG: null ctx, in / ring_offsets / w / out / vertices / face_offsets / normals / bad_rows / index / image / camera, null edge with
 * E > 0, ring with ring_len > 0, triangles / faces / rec / normals with M > 0, T, F, V, width, height < 1, E, ring_len, M < 0, the camera
 * numbers as for nm_mesh_draw; NM_ERR_UNSUPPORTED: V + E >= 2^31, 3 M >= 2^31, F M >= 2^31, F height width >= 2^31. */
int nm_subdiv_apply(nm_ctx* ctx, const double* in, int32_t T, int32_t V, int32_t E, const int32_t* edge, const int32_t* ring_offsets,
                    const int32_t* ring, int32_t ring_len, const double* w, double* out, int32_t* bad_rows);
int nm_vertex_normals(nm_ctx* ctx, const double* vertices, int32_t F, int32_t V, const int32_t* triangles, int64_t M,
                      const int32_t* face_offsets, const int32_t* faces, double* normals, int32_t* bad_rows);
int nm_mesh_shade(nm_ctx* ctx, const double* rec, const int32_t* index, const int32_t* triangles, const double* normals,
                  const double* vertex_colors, const double* color, int32_t F, int32_t V, int64_t M, const nm_camera* camera, double light_a,
                  double light_b, const double* background, uint8_t* image);

/* Evaluation metrics (utils/eval_utils.py).
 * nm_eval_voxel_chamfer — voxel_chamfer_distance :29-55 for every frame of a batch: gt_vox, recon (B,T,1,G,G,G) fp32 on the
 *   device (gt occupied = non-zero, recon occupied = value >= 0.5; neither is modified), per_frame (B*T) fp64 out =
 *   mean_gt min_rec d^2 + mean_rec min_gt d^2 in the reference's [-1,1] coordinates (NaN when a set is empty).  Exact:
 *   integer Euclidean distance transforms instead of the (N,M) distance matrix.
 * nm_eval_semantic — the nearest-keypoint votes of semantic_scores :59-90: keypoints (BT,K,4), gt_keypoints (BT,Kg,3);
 *   closest (BT,Kg) int32 out, counts (Kg,K) int64 ACCUMULATED (caller zeroes it for a new epoch). */
int nm_eval_voxel_chamfer(nm_ctx* ctx, const float* gt_vox, const float* recon, int32_t B, int32_t T, int32_t G, double* per_frame);
int nm_eval_semantic(nm_ctx* ctx, const float* keypoints, const float* gt_keypoints, int32_t BT, int32_t K, int32_t Kg,
                     int32_t* closest, int64_t* counts);

/* Skeleton handed to the VRNN entry points (result of process_affinity_glob,
 * utils/dyna_utils.py:6-171, computed on the host by neural_marionette_amd.skeleton):
 *  parents (K) int32, parents[root] == root;  order (K) int32 = priority.indices */
int nm_vrnn_set_tree(nm_ctx* ctx, const int32_t* parents_host, const int32_t* order_host);

/* HSVRNNBVH.get_offset — model/hsvrnn_bvh.py:236-253.  keypoints (B,T,K,4) -> offset (B,K,3) */
int nm_vrnn_offsets(nm_ctx* ctx, const float* keypoints, int32_t B, int32_t T, float* offset);

/* HSVRNNBVH.encode — model/hsvrnn_bvh.py:67-156.
 *  keypoints (B,T,K,4) in; eps (T,S,B,Z) standard-normal draws in t order (required);
 *  kypt_recon (B,T,K,4), R (B,T,K,3,3), z (B,T,Z), h (B,T+1,H) out;
 *  scalars2: kl_kypt (mean), kypt_recon_loss (mean);  best_idx (B,T) int32 out or NULL. */
int nm_vrnn_encode(nm_ctx* ctx, const float* keypoints, const float* eps, int32_t B, int32_t T,
                   int32_t S, float* kypt_recon, float* R, float* z, float* h, float* scalars2,
                   int32_t* best_idx);

/* ---- training, learner mode (pretrained_mode = 1: detector frozen, train.py:146) -------------------------
 * nm_vrnn_encode_train = nm_vrnn_encode + a ctx-owned tape of the activations the backward pass needs.
 * nm_vrnn_encode_backward back-propagates L = c_rec * kypt_recon_loss + c_kl * kl_kypt through time
 * (dscal2 = device pointer to [dL/dkl_kypt, dL/dkypt_recon_loss], i.e. the loss weights as autograd hands
 * them over) and overwrites the gradient buffers named like the reference's dyna_module parameters
 * (all 21 trainable tensors; offset_param has requires_grad = False, hsvrnn_bvh.py:64-65).
 * nm_adam_step is torch.optim.Adam's update (no weight decay / amsgrad) for one flat tensor. */
typedef struct nm_named_grad {
    const char* name;        /* state_dict key, e.g. "dyna_module.kypt_rnn_cell.weight_ih" */
    float* data;             /* device pointer, same shape as the parameter, overwritten */
    int64_t numel;
} nm_named_grad;
int nm_vrnn_encode_train(nm_ctx* ctx, const float* keypoints, const float* eps, int32_t B, int32_t T,
                         int32_t S, float* kypt_recon, float* R, float* z, float* h, float* scalars2,
                         int32_t* best_idx);
int nm_vrnn_encode_backward(nm_ctx* ctx, const float* dscal2, const nm_named_grad* grads, int32_t count);
int nm_adam_step(nm_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                 int32_t step, float lr, float beta1, float beta2, float eps);
/* the same update for `count` tensors in ONE launch (host arrays of device pointers; torch.optim.Adam semantics per tensor) */
int nm_adam_step_multi(nm_ctx* ctx, float* const* params, const float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const int64_t* numels, int32_t count, int32_t step, float lr,
                       float beta1, float beta2, float eps);
/* the same with a device-side guard: `ok` points to ONE float on the device (written earlier on the ctx stream, e.g. "every gradient
 * is finite"); 0.0f makes the launch a no-op - parameters, exp_avg and exp_avg_sq untouched, no host synchronisation - anything
 * else (or a null pointer) applies the update.  The trainers of train.py pass the finiteness of their gradient bucket. */
int nm_adam_step_multi_ok(nm_ctx* ctx, float* const* params, const float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const int64_t* numels, int32_t count, int32_t step, float lr,
                       float beta1, float beta2, float eps,
                          const float* ok);

/* ---- training, detector mode (pretrained_mode = 0: train.py:270-276, the detector trains on its 11 losses) ----
 * nm_ctx_set_training(ctx, 1) makes nm_ctx_set_weights also pack the weights of the data-gradient convolutions
 * (flipped / transposed copies); it invalidates the current weights, so call nm_ctx_set_weights afterwards.
 * nm_detector_forward_train = nm_detector_forward, but every activation stays in a ctx-owned arena (sized once for
 * forward + backward) together with a tape of the layer sequence.  The caller keeps vox, keypoints and recon alive
 * and unchanged until the backward call.
 * nm_detector_backward back-propagates L = sum_i dlosses11[i] * loss_i (dlosses11: DEVICE vector, the loss weights as
 * autograd hands them over; order as losses11) through the decoder, the losses, the heads and both feature nets
 * (= autograd of kypt_detector.py:81-169 under train.py:388-404) and overwrites the gradient buffers named like the
 * reference's kypt_detector.* parameters (all 315 of them must be present; layouts as in the state_dict). */
int nm_ctx_set_training(nm_ctx* ctx, int32_t on);
int nm_detector_forward_train(nm_ctx* ctx, const float* vox, int32_t B, int32_t T, int32_t affinity_on,
                              float* keypoints, float* heatmaps, float* first_feature, float* recon,
                              float* affinity, float* losses11);
int nm_detector_backward(nm_ctx* ctx, const float* dlosses11, const nm_named_grad* grads, int32_t count);
/* Optional hook for overlapping the gradient all-reduce (train.py:404 `loss.backward()` followed by the optimizer step; here one
 * collective per bucket chunk): a caller-owned hipEvent_t that the next nm_detector_backward calls record once every
 * kypt_detector.kypt_to_vox.* gradient has been written - the decoder's parameters come first in the backward order, the
 * heads and both feature nets follow.  The event is recorded on a ctx-owned stream (the one the weight gradients run on, behind the
 * ctx stream's walk through the decoder): wait for it with hipStreamWaitEvent / hipEventSynchronize, do not assume it orders anything
 * else on the ctx stream.  When nm_detector_backward returns, all of its work is ordered before anything enqueued on the ctx stream
 * afterwards.  NULL removes the hook. */
int nm_ctx_set_backward_event(nm_ctx* ctx, void* hip_event);

/* HSVRNNBVH.generate — model/hsvrnn_bvh.py:158-234.
 *  keypoints_cond (B,Tcond,K,4); eps_post (Tcond,S,B,Z); eps_prior (Ttot-Tcond,B,Z);
 *  out_cond (B,Tcond,K,4), out_gen (B,Ttot-Tcond,K,4); h_last (B,H) or NULL. */
int nm_vrnn_generate(nm_ctx* ctx, const float* keypoints_cond, const float* eps_post,
                     const float* eps_prior, int32_t B, int32_t Tcond, int32_t Ttot, int32_t S,
                     float* out_cond, float* out_gen, float* h_last);

/* Prior rollout from a given state — the generation loop of vis_generation.py:117-127 (per step: extract_prior_dist, rsample,
 * extract_kypt_from_latent_and_state, kypt_rnn_cell) for T steps in one call:
 *  h_in (B,H), offset (B,K,3) [get_offset], eps (T,B,Z); kp_out (B,T,K,4); h_out (B,H) or NULL.
 * For batches <= 64 rows this and nm_vrnn_generate replay a HIP graph of their launch sequence, captured on first use per
 * (B, Tcond, T) and kept in the context (three dependent launches per prior step; NM355_VRNN_GRAPH=0 enqueues them one by one). */
int nm_vrnn_rollout(nm_ctx* ctx, const float* h_in, const float* offset, const float* eps, int32_t B, int32_t T,
                    float* kp_out, float* h_out);

/* One VRNN step for hand-rolled rollouts (vis_generation.py:97-127 of the reference):
 *  posterior != 0: best-of-S posterior step against kp_obs (B,K*4), eps (S,B,Z);
 *  posterior == 0: prior step, eps (B,Z), S ignored.
 *  h_in (B,H), offset (B,K,3) -> kp_out (B,K*4), z_out (B,Z), h_out (B,H) (NULL: skip the GRU update). */
int nm_vrnn_step(nm_ctx* ctx, int32_t posterior, const float* h_in, const float* kp_obs,
                 const float* offset, const float* eps, int32_t B, int32_t S, float* kp_out,
                 float* z_out, float* h_out);

/* idx = argmin over rows r of || rows[r] - target[r*target_row_stride] ||^2 (first minimum; stride 0 =
 * one target for all rows): the sample selection of vis_generation.py:109-110 / vis_interpolation.py:113-119.
 *  rows (B,D), target (D) or (B,D), idx_out (1) int32 on the device, dist_out (1) or NULL. */
int nm_rows_argmin_dist(nm_ctx* ctx, const float* rows, const float* target, int32_t target_row_stride,
                        int32_t B, int32_t D, int32_t* idx_out, float* dist_out);

/* ---- motion retargeting (vis_retarget.py of the reference, the computation between its two detector calls and its first render) ----
 * Bind a target point cloud to the skeleton once, then pose it for T frames.  All three calls use the tree of nm_vrnn_set_tree
 * (parents, order, root = order[0]) and fail with NM_ERR_STATE when none is set, NM_ERR_ARG when K is not the context's nkeypoints or
 * N < 1 / T < 1.  Point data is float64 like the reference's numpy points; `w`, `local` and `out` must be 16-byte aligned.  Results are
 * bit-identical from run to run (no atomics).
 *
 * nm_retarget_bind - extract_skin_weights (vis_retarget.py:21-62) and the local coordinates of :268-270 in one pass over the points.
 *   points (N,3) float64, keypoints (K,4) fp32, R_bind (K,3,3) fp32 or NULL (identity), force_child (N) int32 or NULL: imposes the
 *   selection (values in [0,K): the caller checks; `margin` is still the free selection's).
 *   child (N) int32 = the joint whose bone point is nearest (first minimum), parent (N) int32 = parents[child] of the ORIGINAL tree,
 *   w (N,2) fp32 = weight of the child joint, weight of the parent joint, local (N,2,3) float64 = R_bind[j]^T (p - pos_j) for
 *   j = child, parent, margin (N) float64 or NULL = second-smallest minus smallest bone distance, dense (N,K) fp32 or NULL = the
 *   reference's matrix.  Operation by operation as the reference: invalid[k] = intensity_k < (float)threshold in fp32; bone point of
 *   joint k in fp32 = the joint for the root, else (pos_k + pos_a) / 2 with a the nearest ancestor that is not invalid; distances in
 *   float64, sqrt((dx dx + dy dy) + dz dz); invalid joints and the root take the distance VALUE 1e4; c = exp(hardness |p - pos_child|),
 *   q = exp(hardness |p - pos_parent|), w_child = (float)(q / (c + q)), w_parent = (float)(c / (c + q)).  When the root is chosen
 *   (every joint masked) parent == child: the reference's second assignment overwrites the first, so the dense row holds w_child alone
 *   and w_parent is written as 0.
 *   The ancestor walk STOPS AT THE ROOT even when the root is invalid, after at most K steps: the reference's loop (:41-42) does not
 *   terminate in that case (parents[root] == root), so this is the library's own choice, not a reference behaviour.
 * nm_retarget_fk - the re-posing loop of :275-300: R (T,K,3,3), root_pos (T,3), offset (K,3) [nm_vrnn_offsets] -> pos (T,K,3):
 *   pos[root] = root_pos, pos[j] = R[j] offset[j] + pos[parents[j]] in `order`, fp32, then clipped to [-1, 1].
 * nm_retarget_pose - the blend of :303-322 on the bind record: out (T,N,3) float64,
 *   out[t,n] = w_child (R[t,child] local_child + pos[t,child]) + w_parent (R[t,parent] local_parent + pos[t,parent]); the parent term is
 *   0 when parent == child. */
int nm_retarget_bind(nm_ctx* ctx, const double* points, int64_t N, const float* keypoints, const float* R_bind, int32_t K, double hardness,
                     double threshold, const int32_t* force_child, int32_t* child, int32_t* parent, float* w, double* local,
                     double* margin, float* dense);
int nm_retarget_fk(nm_ctx* ctx, const float* R, const float* root_pos, const float* offset, int32_t T, int32_t K, float* pos);
int nm_retarget_pose(nm_ctx* ctx, const int32_t* child, const int32_t* parent, const float* w, const double* local, const float* R,
                     const float* pos, int32_t T, int64_t N, int32_t K, double* out);

/* Sub-module callables the reference's demo scripts reach into (hsvrnn_bvh.py:29-57):
 *  which: 0 extract_post_dist (H+K*4 -> 2Z), 1 extract_prior_dist (H -> 2Z),
 *         2 root_intensity_decoder (H+Z -> 3+K, tanh), 3 joint_matrix_decoder (H+Z -> 6K) */
int nm_vrnn_mlp(nm_ctx* ctx, int32_t which, const float* x, int32_t B, float* y);
/* kypt_rnn_cell: x (B,K*4+Z), h (B,H) -> h_out (B,H) */
int nm_vrnn_gru(nm_ctx* ctx, const float* x, const float* h, int32_t B, float* h_out);
/* extract_kypt_from_latent_and_state — hsvrnn_bvh.py:255-286: dec_in (B,H+Z), offset (B,K,3)
 *  -> kp (B,K*4), R (B,K,3,3) */
int nm_vrnn_fk(nm_ctx* ctx, const float* dec_in, const float* offset, int32_t B, float* kp, float* R);

/* ---- op-level entry points (unit parity tests; activations are channels-last) ------------ */
/* Conv3d.  in [N][D][H][W][Cin8] (Cin8 = Cin rounded up to 8, extra channels zero), weight in
 * torch OIDHW layout, out [N][OD][OH][OW][Cout].  in_scale/in_shift [N][Cin8] or NULL apply
 * y = lrelu_slope(x*scale+shift) to the input first.  If gn_groups > 0, also returns the
 * following GroupNorm's per-(n,c) scale/shift (gn_gamma/gn_beta [Cout]) in gn_scale/gn_shift.
 * up2 != 0: `in` is at half resolution and its trilinear x2 upsampling (align_corners=False) is
 * what gets convolved (nn.Upsample fused into the conv, kypt_detector.py:427-429,441-444). */
int nm_op_conv3d(nm_ctx* ctx, const float* in, int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin,
                 const float* in_scale, const float* in_shift, float in_slope,
                 const float* weight, const float* bias, int32_t Cout, int32_t ks, int32_t stride,
                 int32_t pad, float* out, int32_t gn_groups, const float* gn_gamma,
                 const float* gn_beta, float* gn_scale, float* gn_shift, int32_t up2);
/* First layer of a feature net (kypt_detector.py:265): Conv3d(1+3 -> Cout, k5, p2) on
 * cat[occ, coord ramps] evaluated as conv(occ) + weight-only constant field.  occ [N][G][G][G],
 * weight (Cout,4,5,5,5) OIDHW, out [N][G][G][G][Cout] (+ following GroupNorm as in nm_op_conv3d). */
int nm_op_conv5_occ(nm_ctx* ctx, const float* occ, int32_t N, int32_t G, const float* weight,
                    const float* bias, int32_t Cout, float* out, int32_t gn_groups,
                    const float* gn_gamma, const float* gn_beta, float* gn_scale, float* gn_shift);
int nm_op_convT2(nm_ctx* ctx, const float* in, int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin,
                 const float* weight_iodhw, const float* bias, int32_t Cout, int32_t outpad, float* out,
                 int32_t gn_groups, const float* gn_gamma, const float* gn_beta, float* gn_scale,
                 float* gn_shift);
/* out = T_a(a) + T_b(b) with T(x) = lrelu_slope(x*scale+shift); b may be NULL */
int nm_op_apply2(nm_ctx* ctx, const float* a, const float* a_scale, const float* a_shift, float a_slope,
                 const float* b, const float* b_scale, const float* b_shift, float b_slope,
                 int32_t N, int32_t voxels, int32_t C, float* out);
int nm_op_upsample2(nm_ctx* ctx, const float* in, int32_t N, int32_t D, int32_t H, int32_t W, int32_t C, float* out);
int nm_op_pack_input(nm_ctx* ctx, const float* vox, int32_t B, int32_t T, int32_t G, int32_t mean_over_t, float* out);
int nm_op_cl_to_ncdhw(nm_ctx* ctx, const float* in, int32_t N, int32_t voxels, int32_t C, float* out);
/* Backward ops (detector-mode training, train.py:388-404 = autograd of the modules above; unit parity in
 * tests/test_grad_ops_gpu.py).  Tensors are channels-last like the forward ops.
 * nm_op_conv3d_backward: y = conv3d(up2 ? upsample2(a) : a, W) + b with a = lrelu(in*scale+shift) (vox_modules.py:12,27,31,53;
 *   kypt_detector.py:427-445).  d_weight is OIDHW, d_bias = sum dy, d_in = dL/da for the first dgrad_channels input
 *   channels [N][D][H][W][dgrad_channels] (NULL: skipped).  The data gradient is the forward conv kernel on flipped /
 *   transposed weights (stride 1), the transposed-conv kernel (k2 s2), plus the adjoint of the trilinear upsampling (up2).
 * nm_op_conv5_occ_backward: weight / bias gradients of the first layer conv5(cat[occ, coords]) (kypt_detector.py:265).
 * nm_op_convT2_backward: ConvTranspose3d(k2, s2, output_padding) of vox_modules.py:68; weight IODHW.
 * nm_op_gn_backward: GroupNorm(groups, eps 1e-5) + LeakyReLU(slope) on the raw tensor y: dy, dgamma, dbeta and sum_v dy. */
int nm_op_conv3d_backward(nm_ctx* ctx, const float* in, int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin,
                          const float* in_scale, const float* in_shift, float in_slope, const float* weight, int32_t Cout,
                          int32_t ks, int32_t stride, int32_t pad, int32_t up2, const float* dy, float* d_in,
                          int32_t dgrad_channels, float* d_weight, float* d_bias);
int nm_op_conv5_occ_backward(nm_ctx* ctx, const float* occ, int32_t N, int32_t G, int32_t Cout, const float* dy,
                             float* d_weight, float* d_bias, int32_t sparse_occ /* occupancy channel: 1 = matrix cores over the non-empty 4x8x8 bricks (the gather when G % 8 != 0), 2 = gather over the occupied voxels, 0 = generic dense kernel */);
int nm_op_convT2_backward(nm_ctx* ctx, const float* in, int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin,
                          const float* in_scale, const float* in_shift, float in_slope, const float* weight, int32_t Cout,
                          int32_t outpad, const float* dy, float* d_in, float* d_weight, float* d_bias);
int nm_op_gn_backward(nm_ctx* ctx, const float* y, int32_t N, int32_t voxels, int32_t C, int32_t groups, const float* gamma,
                      const float* beta, float slope, const float* dA, float* dy, float* dgamma, float* dbeta, float* dbias);
/* Detector heads and losses, one launcher sequence of the network path per call on tensors the caller chooses (unit parity against
 * fp64 in tests/test_heads_ops_gpu.py).  Scratch comes from the context's workspace: do not interleave with a network call whose
 * results are still being read.  F = B T frames, g = heat-map edge, G = occupancy-grid edge, dloss = device vector of 11 loss weights
 * (order of losses11).  Outputs the launchers accumulate into (dkp, dfeat) are zeroed by the call.
 * nm_op_heatmaps[_backward]: head (F,g,g,g,Kc) / clip_head (B,g,g,g,Kc) channels-last head outputs (Kc >= K, Kc % 4 == 0), prop (3) =
 *   propagate weight 0, 1, bias; recurrent 0 = const_intensity 3, 1 = const_intensity 2 -> heatmaps (F,K,g,g,g), keypoints (F,K,4),
 *   heat_mean (F,K).  Backward: dkp (F,K,4) and dloss[4] (sparsity) -> dhead, dclip_head (layouts of head / clip_head), dprop (3).
 * nm_op_combined[_backward]: Gaussian table (F,K,3,g; `table` may be NULL) of width 2 (sigma / g)^2, or per keypoint from sigma_param (K)
 *   (fixed_sigma = 0: sigmoid(p) 2 sigma), and the combined representation out (F,g,g,g,Cc) = [gauss_t K | first_feature Fd | gauss_0 K |
 *   3 coordinates | zeros]; first_feature (B,g,g,g,Fd); cat 0 / 1 / 2 = gaussian_cat_type none / max / sum.  Backward: dcomb (F,g,g,g,Cd) ->
 *   dfeat (F,g,g,g,Fd) (frame 0 of every clip holds the clip's sum, the rest zeros), dkp (F,K,4), dsigma_param (K, with sigma_param).
 * nm_op_decoder_tail[_backward]: x (F,G,G,G,C) raw with per-frame scale / shift (F,C) and LeakyReLU slope, w14 (C+1: weights, bias),
 *   first_frames: frame b ff_stride_frames is clip b's, target / keypoints may be NULL -> recon (F,G,G,G), frame_sums (F,3) = BCE sum,
 *   occupancy-masked chamfer sum, occupied count.  Backward (dloss[0], dloss[1]): dA (F,G,G,G,C), or with dvout (F,G,G,G; C == 32) only the
 *   per-voxel factor (dA = dvout (x) w14[0..C)), dw14 (C+1), and with dkp (F,K,4) the chamfer term's keypoint gradient.
 * nm_op_clip_losses[_backward]: the 11 losses from keypoints (F,K,4), affinity (N,K,K) or NULL, heat_mean (F,K), frame_sums (F,3) and
 *   vol_override (F,2) or NULL (numerator, denominator of vol_fit 'gaussian'); vol_fit 0 writes a zero volume term.  Backward: dkp (F,K,4)
 *   and dinfl (B,K,K) (with an affinity) of the separation, local, time and trajectory terms.
 * nm_op_affinity[_backward]: get_affinity version 0-3 from params (N,K,K-1) [3] / (N,K,K) -> (N,K,K); backward from dinfl (B,K,K) and
 *   dloss[7] (neighbour sparsity) -> dparams.
 * nm_op_volfit_gauss[_backward]: vol_fit_type 'gaussian': vox (F,G,G,G), keypoints -> vol (F,2); backward dloss[1] -> dkp (F,K,4). */
int nm_op_heatmaps(nm_ctx* ctx, const float* head, const float* clip_head, const float* prop, int32_t B, int32_t T, int32_t K, int32_t Kc,
                   int32_t g, int32_t recurrent, float* heatmaps, float* keypoints, float* heat_mean);
int nm_op_heatmaps_backward(nm_ctx* ctx, const float* head, const float* clip_head, const float* prop, int32_t B, int32_t T, int32_t K,
                            int32_t Kc, int32_t g, int32_t recurrent, const float* dkp, const float* dloss, float* dhead,
                            float* dclip_head, float* dprop);
int nm_op_combined(nm_ctx* ctx, const float* keypoints, const float* first_feature, const float* sigma_param, int32_t B, int32_t T, int32_t K,
                   int32_t Fd, int32_t g, int32_t Cc, float sigma, int32_t cat, float* table, float* out);
int nm_op_combined_backward(nm_ctx* ctx, const float* dcomb, int32_t Cd, const float* keypoints, const float* sigma_param, int32_t B,
                            int32_t T, int32_t K, int32_t Fd, int32_t g, float sigma, int32_t cat, float* dfeat, float* dkp,
                            float* dsigma_param);
int nm_op_decoder_tail(nm_ctx* ctx, const float* x, const float* scale, const float* shift, float slope, int32_t B, int32_t T, int32_t C,
                       int32_t G, const float* w14, const float* first_frames, int32_t ff_stride_frames, const float* target,
                       const float* keypoints, int32_t K, float* recon, float* frame_sums);
int nm_op_decoder_tail_backward(nm_ctx* ctx, const float* x, const float* scale, const float* shift, float slope, int32_t F, int32_t C, int32_t G,
                                const float* w14, const float* target, const float* recon, const float* frame_sums, const float* keypoints,
                                int32_t K, const float* dloss, float* dA, float* dvout, float* dw14, float* dkp);
int nm_op_clip_losses(nm_ctx* ctx, const float* keypoints, const float* affinity, const float* heat_mean, const float* frame_sums,
                      const float* vol_override, int32_t B, int32_t T, int32_t K, int32_t N, int32_t G, float sep_sigma, int32_t graph_ver,
                      int32_t graph_flags, int32_t use_traj, int32_t vol_fit, float* losses11);
int nm_op_clip_losses_backward(nm_ctx* ctx, const float* keypoints, const float* affinity, const float* dloss, int32_t B, int32_t T, int32_t K,
                               int32_t N, float sep_sigma, int32_t graph_ver, int32_t graph_flags, int32_t use_traj, float* dkp,
                               float* dinfl);
int nm_op_affinity(nm_ctx* ctx, const float* params, int32_t N, int32_t K, int32_t ver, float* affinity);
int nm_op_affinity_backward(nm_ctx* ctx, const float* params, const float* affinity, const float* dinfl, const float* dloss, int32_t B, int32_t N,
                            int32_t K, int32_t ver, int32_t graph_ver, int32_t graph_flags, float* dparams);
int nm_op_volfit_gauss(nm_ctx* ctx, const float* vox, const float* keypoints, int32_t B, int32_t T, int32_t K, int32_t G, float sigma,
                       float* vol);
int nm_op_volfit_gauss_backward(nm_ctx* ctx, const float* vox, const float* keypoints, const float* dloss, int32_t B, int32_t T, int32_t K,
                                int32_t G, float sigma, float* dkp);
/* The two lowest hourglass levels of one feature net (vox_modules.py:78-120: encoder_res2, skip_res3, encoder_pool3, encoder_res3,
 * decoder_res3, decoder_upsample3 + skip, decoder_res2) with the weights nm_ctx_set_weights loaded; unit parity against fp64 in
 * tests/test_hgcore_gpu.py.  which: 0 = the frame feature net's hourglass, 1 = the clip-mean net's.  in [N][D^3][32] channels-last is the
 * pool-2 output, its pending GroupNorm + LeakyReLU as per-frame in_scale / in_shift [N][32] and in_slope (both NULL and slope 1: `in` is
 * already activated); out [N][D^3][48] plain fp32.  The transposed conv's output_padding is D % 2; the context's grid_size plays no part.
 * fused = 1: the one-launch form of the inference forward (hg_core_kernel); NM_ERR_UNSUPPORTED, never a fall-back, where it is not
 * eligible - conv mode other than 1, a layer without a split-fp16 pack, D outside 2 .. 6, tensors that do not fit in LDS.  fused = 0: the
 * same layers as the separate launches of the inference forward without the core (D 2 .. 64).  Neither form looks at NM355_HG_CORE.
 * NM_ERR_ARG: null ctx / in / out, only one of in_scale / in_shift, which or fused not 0 / 1, N < 1, D < 1.  Scratch comes from the
 * context's workspace; the range guard's status word is left alone (a non-finite result is in `out` for the caller to see). */
int nm_op_hourglass_core(nm_ctx* ctx, int32_t which, const float* in, const float* in_scale, const float* in_shift,
                         float in_slope, int32_t N, int32_t D, int32_t fused, float* out);
/* Conv arithmetic (per context: two contexts in one process may run in different modes; like every other launch-time
 * switch it lives in the nm_ctx).  mode 0: exact fp32 MFMA (v_mfma_f32_32x32x2_f32) for every conv.
 * mode 1 (default): layers with Cin % 16 == 0 run on the fp16 matrix cores with every fp32 operand split
 * into fp16 hi + lo*2^-11 and three products x_hi*w_hi + 2^-11 (x_hi*w_lo + x_lo*w_hi) accumulated in
 * fp32 — error within one fp32 rounding of the exact product, same tolerance class as the fp32 fma
 * chain, 16x/3 the MFMA rate.  mode 2 = mode 1 with the producer/consumer kernel (conv_f16p) on every layer it
 * supports instead of the Cout == 32 layers only (same arithmetic; a test / measurement switch).  Parity tests run in
 * all modes.  mode 3 = reduced precision for training at autocast-class accuracy (BASELINE.json config 3 names bf16): the
 * kernels of mode 1 with only the x_hi*w_hi product, i.e. operands rounded to fp16 (11 significant bits - three more than
 * bf16, same MFMA rate), fp32 accumulation, fp32 tensors, statistics, losses, master weights and optimiser; the layers mode 1
 * leaves on the fp32 cores (k = 1 weight gradients, volumes under 16^3, heads, VRNN) stay fp32.  Forward, data and weight
 * gradients all follow the mode.  Outputs differ from the reference's fp32 path by ~1e-3 relative (tests state the bound);
 * the 1e-4 parity contract holds in modes 0-2 only.
 * mode 4 = BASELINE config 3 as named ("bf16"): mode 3's arithmetic with 16-BIT STORAGE of the training path - every activation the
 * training forward keeps for the backward pass and every activation gradient with at least 32^3 voxels per frame is stored as
 * bfloat16 (8 significant bits, fp32's range: no loss scaling), converted to fp32 on read and rounded to nearest even on write;
 * master weights, GroupNorm statistics / scale / shift, every partial sum and accumulator, the losses and the Adam state stay fp32,
 * as do the tensors below 32^3 (the hourglass, heads, keypoints) and the inference forward (which keeps mode 3's fp32 workspace).
 * Halves the training arena and the bytes of the GroupNorm-backward passes; gradients agree with the fp64 oracle to a few 1e-2 in
 * whole-gradient L2 (tests state the bound).  A training step keeps all B * T frames in one pass, at any frame count: the 3x3x3 weight
 * gradient of bfloat16 operands runs on wgrad16z_kernel alone, whose per-frame scale / shift table in LDS holds 96 frames, so above
 * 96 frames it is launched once per group of at most 96 frames (equal groups, e.g. 240 = 3 x 80), each group on its own partial-sum
 * slots, and one fixed-order reduce sums all slots: no atomics, run-to-run bit-identical, the workspace grows with the group count;
 * up to 96 frames the single launch and its bits are unchanged.  (The fp32-storage modes run wgrad16_kernel above 96 frames.) */
int nm_set_conv_mode(nm_ctx* ctx, int32_t mode);
int nm_get_conv_mode(nm_ctx* ctx);
/* Element type of the tensors the op-level entry points below (nm_op_*) read and write, for unit parity of the 16-bit storage kernels
 * of conv mode 4: in_h != 0 - the tensors on the input side (in / a / y and every gradient of their shape: d_in, dA, dy of
 * nm_op_gn_backward) are bfloat16; out_h != 0 - the tensors on the output side (out, the incoming dy of the backward ops) are.
 * Defaults 0 / 0 (fp32, the element type of every network-level entry point's arguments).  Kernels without an instantiation for the
 * requested combination fail with NM_ERR_UNSUPPORTED. */
int nm_op_set_storage16(nm_ctx* ctx, int32_t in_h, int32_t out_h);

/* ---- live kernel timing for bench.py's roofline leg -------------------------------------------
 * While enabled, every conv launch of this context is bracketed by a HIP event pair.  on = 1: launches on the ctx stream only
 * (launches the library puts on its own side stream overlap the main stream, so their event-to-event time is not their own);
 * on = 2: side-stream launches are recorded too (for listing every kernel family's share; durations include contention).
 * on = 3: as 1, but only launches of >= 20 GFLOP algorithmic work (what bench.py's timed region uses: the event pairs around the
 * many small dependent launches of the coarse hourglass levels cost the step ~1 % and no roofline is read from them).
 * Records belong to the context.
 * nm_prof_read sums duration and ALGORITHMIC flops (2*voxels*Cout*Cin*k^3, un-padded) of one
 * kernel variant (0..3 = conv_mfma_kernel<MT,NT> with (MT,NT) = (1,1),(1,2),(2,1),(2,2); 5,6 =
 * conv_f16s_kernel<2,1>/<2,2> (k1 / k3 without upsampling), 10,11 = the same kernel with the fused trilinear upsampling (NT = 1 / 2),
 * 7 = conv_f16p_kernel, 8 = conv_pool_f16s_kernel, 9 = conv_f16p2_kernel (algorithmic fp32-equivalent flops, i.e. 1/3 of the issued MFMA flops); 4 = the
 * first-layer occupancy kernel conv_k5occ_kernel, credited with the reference's dense 4-channel k5 work; 12 = conv_up2c_kernel (main + shell
 * launches); 13 = wgrad16_kernel, the split-fp16 k3 weight-gradient kernels with their fixed-order reduce (2*voxels*Cout*Cin*27);
 * 14 = conv_f16q2_kernel, the one-product modes' 64-channel conv; 15 = conv_f16r_kernel, their 32-output-channel conv with resident weights).
 * Variant 16 is a count, not a timed family: the launches that the decoder schedule (NM355_ENC_SCHED bits 2 and 4) sent to the library's third
 * stream since nm_prof_enable, in any mode (ms_total and flops_total are 0); 0 means that schedule ran in the serial order. */
int nm_prof_enable(nm_ctx* ctx, int32_t on);
int nm_prof_read(nm_ctx* ctx, int32_t variant, double* ms_total, double* flops_total, int64_t* launches);
const char* nm_prof_kernel_name(int32_t variant);
/* host helper: torch.linspace(-1, 1, n) as the kernels evaluate it */
int nm_host_linspace(int32_t n, float* out_host);

#ifdef __cplusplus
}
#endif
#endif /* NM355_H */
