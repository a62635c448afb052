/*
 * dhaug.h -- C-ABI of libdhaug.so: hand-written HIP (gfx950 / MI355X) kernels for the DH-AUG hot path
 * (DH forward kinematics + MLP GAN generator / critic step).
 *
 * The reference (R/ = DH-AUG_master/) is pure Python on stock PyTorch ops; it has no FFI layer.  Each entry
 * point below therefore names the reference *Python* symbol whose arithmetic it replaces (file:line).  The
 * Python drop-in classes in the package bind these through ctypes.
 *
 * Conventions
 *   - plain C: raw device pointers + sizes; no torch / C++ types cross the boundary.
 *   - the caller owns every buffer; the library allocates nothing and keeps no state.
 *   - all work is enqueued on the caller's HIP stream (`stream`, a hipStream_t passed as void*); no
 *     synchronisation inside, safe for hipGraph capture.
 *   - return value: 0 on success; a negative DHAUG_E* code for an argument error detected on the host
 *     (nothing was launched); a positive hipError_t value if the launch failed.  Never throws.
 *   - fp32 tensors are contiguous row-major.  bf16 tensors are row-major with an explicit leading dimension
 *     (elements); rows must start 16-byte aligned (ld % 8 == 0, base 16-byte aligned).
 *   - angle layout (degrees), 37 columns = `generator_angle` of R/models_Fk_GAN/Fk_generator.py:179-186:
 *       [0:5] right leg, [5:10] left leg, [10:23] body, [23:28] right arm, [28:33] left arm,
 *       [33] unused, [34:37] global rotation x,y,z.
 *   - bone_len layout, 15 columns = used_16key_15bone_len_table order
 *       (R/models_Fk_GAN/forward_kinematics_DH_model.py:46-49).
 *   - out16 = the 16 H36M joints of R/common/h36m_dataset.py:37-38, (N,16,3).
 */
#ifndef DHAUG_H
#define DHAUG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DHAUG_VERSION 100            /* major*10000 + minor*100 + patch */

#define DHAUG_OK             0
#define DHAUG_EINVAL        -1       /* null pointer / negative size / bad enum */
#define DHAUG_EALIGN        -2       /* pointer or leading dimension violates the alignment contract */
#define DHAUG_EUNSUPPORTED  -3       /* shape outside what the kernels implement */

/* activation kinds for dhaug_gemm_bf16 epilogues */
#define DHAUG_ACT_NONE   0
#define DHAUG_ACT_RELU   1
#define DHAUG_ACT_LRELU  2           /* LeakyReLU, slope passed separately (reference uses 0.01) */

int dhaug_version(void);
/* name of the code-object architecture the library was built for ("gfx950") */
const char* dhaug_arch(void);

/* ------------------------------------------------------------------------------------------------------
 * Forward kinematics
 * ---------------------------------------------------------------------------------------------------- */

/* Fused DH forward kinematics: 33 local DH matrices, 5 chain products, global rotation, root add,
 * 32->16 joint gather -- one kernel, one HBM read of the inputs, one write of the joints.
 * Replaces Forward_Kinematics_DH_Model.change_3d_joint_angle (torch branch)
 *   R/models_Fk_GAN/forward_kinematics_DH_model.py:562-822 (+ dh_matrix :80-116, rotationMatrix :141-191)
 * followed by the H36M_32_To_16_Table gather of R/models_Fk_GAN/Fk_generator.py:259.
 *   angles (N,37) deg, bone_len (N,15) m, root (N,3) m  ->  out (N,out_joints,3), out_joints in {16,32}.
 * out_joints == 32 reproduces the reference's (N,32,3) tensor exactly (unused rows = root).
 * root may be NULL (= zeros).  Here and in the four entries below, every input (grad_out16 / grad_fake16 included) and the
 * outputs out, fake16, centered, kcs_bf16, proj2d and scaler_out move as 16-byte vectors and must be 16-byte aligned
 * (DHAUG_EALIGN, checked before the launch; optional pointers where non-NULL); the gradient outputs and angles_out need 4 bytes.
 * One workgroup (one wave) takes tiles of 64 poses, at most DHAUG_FK_MAX_BLOCKS workgroups per launch (the four-wave
 * dhaug_gen_tail_forward_critics: DHAUG_GEN_TAIL4_MAX_BLOCKS): more tiles, more trips of a workgroup's tile loop. */
#define DHAUG_FK_MAX_BLOCKS 10240
#define DHAUG_GEN_TAIL4_MAX_BLOCKS 4096
int dhaug_fk_forward(const float* angles, const float* bone_len, const float* root, float* out,
                     int64_t N, int out_joints, void* stream);

/* Reverse-mode gradient of dhaug_fk_forward(out_joints=16) w.r.t. all three inputs (the G step
 * back-propagates through FK: R/models_Fk_GAN/model_fk_gan_train.py:431-480).
 *   grad_out16 (N,16,3) -> grad_angles (N,37), grad_bone_len (N,15), grad_root (N,3).
 * grad_angles columns that cannot move any joint (4,9,22,27,32,33) are written as 0. */
int dhaug_fk_backward(const float* angles, const float* bone_len, const float* grad_out16,
                      float* grad_angles, float* grad_bone_len, float* grad_root, int64_t N, void* stream);

/* Generator tail fused in front of FK: tanh on the 35 head columns (x10 on the root columns), scatter of the
 * 31 live columns into the 37 angle slots, joint-limit affine map (use_preangle) or x180, bone-length
 * jitter len*(1+s[pair]), FK, 32->16 gather.
 * Replaces R/models_Fk_GAN/Fk_generator.py:121-259 (Fk_Generator.forward after deconv_out) and :310-453.
 *   head (N,35) fp32 pre-activation, bone_len (N,15), scaler (N,8) (may be NULL = no jitter)
 *   -> fake16 (N,16,3); angles_out (N,37) optional (NULL to skip) = `generator_angle`. */
int dhaug_gen_tail_forward(const float* head, const float* bone_len, const float* scaler, float* fake16,
                           float* angles_out, int64_t N, int use_preangle, void* stream);

/* dhaug_gen_tail_forward that also emits what the critics consume, while the joints are still in registers:
 *   centered (N,16,3) = fake16 - fake16[:,0]                      (R/models_Fk_GAN/model_fk_gan_train.py:312)
 *   kcs_bf16 (N,32) bf16 = special_KCS_Input_transform(fake16) zero-padded (Fk_discriminator.py:36-146; the operand of
 *                          dhaug_kcs_forward / dhaug_mlp_forward)
 *   proj2d   (N,16,2)   = project_to_2d(GAN_torch_world_to_camera(fake16, quat, trans), cam9)   (:374-376;
 *                          quat[4], trans[3], cam9[9] host arrays as in dhaug_world_to_camera_project)
 * Any of the three may be NULL.  draw_scaler != 0 (scaler must be NULL): the bone-length jitter
 * `randint(-200, 200, (N, 8)) / 1000` (Fk_generator.py:196-203) is drawn inside the kernel with Philox4x32-10 keyed by
 * rng_seed, counter (pose index, rng_offset); scaler_out (N,8), if given, receives the draw.
 *   The draw of pose i (its row index in this call, 64 bits) is two Philox calls, half h in {0, 1}:
 *     counter c0, c1 = low, high 32 bits of i;  c2, c3 = low, high 32 bits of the 64-bit sum rng_offset + h (it wraps at 2^64);
 *     key k0, k1 = low, high 32 bits of rng_seed;  result r[0..3].
 *   Half 0 feeds columns 0..3, half 1 columns 4..7: column 4 h + q = ((int)(r[q] mod 400) - 200) / 1000, the division correctly
 *   rounded in fp32.  Calls whose offsets differ by at least 2 share no counter.
 * inputs_bf16 != 0: centered and proj2d are written as bf16 (N,48) / (N,32) -- the rounding the critics' first layer
 * applies to them anyway (dhaug_mlp_forward LOAD units), at half the bytes. */
int dhaug_gen_tail_forward_critics(const float* head, const float* bone_len, const float* scaler, float* fake16,
                                   void* centered, uint16_t* kcs_bf16, const float* quat, const float* trans,
                                   const float* cam9, void* proj2d, int draw_scaler, uint64_t rng_seed,
                                   uint64_t rng_offset, float* scaler_out, int64_t N, int use_preangle, int inputs_bf16,
                                   void* stream);

/* Gradient of dhaug_gen_tail_forward w.r.t. head: grad_fake16 (N,16,3) -> grad_head (N,35)
 * (column 31 = 0).  Recomputes the forward from head. */
int dhaug_gen_tail_backward(const float* head, const float* bone_len, const float* scaler,
                            const float* grad_fake16, float* grad_head, int64_t N, int use_preangle,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Pose features
 * ---------------------------------------------------------------------------------------------------- */

/* Bone lengths of 16-joint poses: (N,16,3) -> (N,15).  Replaces
 * Fk_Generator.GAN_generator_get_bone_length, R/models_Fk_GAN/Fk_generator.py:107-111
 * (Fk_get_boneVecByPose3d, R/models_Fk_GAN/special_operate.py:513-539, + norm). */
int dhaug_bone_length(const float* pose16, float* bone_len, int64_t N, void* stream);

/* KCS features: 15 adjacent-bone cosines (+ the 15 bone lengths when with_lengths != 0).
 * Replaces special_KCS_Input_transform R/models_Fk_GAN/Fk_discriminator.py:36-146 and the video variant
 * :269-377.  pose16 (N,16,3) fp32.
 *   out_f32 : optional (N, 30|15) fp32, contiguous.
 *   out_bf16: optional (N, ld_bf16) bf16 with columns [30|15, ld_bf16) zero-filled (GEMM operand). */
int dhaug_kcs_forward(const float* pose16, float* out_f32, uint16_t* out_bf16, int64_t ld_bf16,
                      int64_t N, int with_lengths, void* stream);

/* The 3D critic's two inputs in one pass over the pose: centered (N,16,3) = pose16 - pose16[:,0] (the
 * `inputs_3d - inputs_3d[:, :1]` at R/models_Fk_GAN/model_fk_gan_train.py critic calls) and the bf16 KCS operand of
 * dhaug_kcs_forward (KCS is translation invariant, so it is the same feature the critic computes from `centered`). */
int dhaug_center_kcs_forward(const float* pose16, float* centered, uint16_t* out_bf16, int64_t ld_bf16,
                             int64_t N, int with_lengths, void* stream);

/* VJP of dhaug_kcs_forward: grad_feat (N,30|15) fp32 -> grad_pose16 (N,16,3). */
int dhaug_kcs_backward(const float* pose16, const float* grad_feat, float* grad_pose16, int64_t N,
                       int with_lengths, void* stream);

/* JVP (forward-mode) of dhaug_kcs_forward along tangent (N,16,3): -> tan_feat (N,30|15).  Used by the
 * analytic WGAN-GP gradient (R/models_Fk_GAN/Fk_discriminator.py:205-231 with create_graph=True). */
int dhaug_kcs_jvp(const float* pose16, const float* tangent, float* tan_feat, int64_t N, int with_lengths,
                  void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Camera / projection ("next" row N1): between the FK output and the 2D critic on every iteration
 * ---------------------------------------------------------------------------------------------------- */

/* world -> camera by quaternion (qinverse, qrot) + H36M non-linear projection, one shared camera.
 * Replaces GAN_torch_world_to_camera R/common/camera.py:36-38 (+ R/common/quaternion.py:6-35) and
 * project_to_2d R/common/camera.py:62-94 as called at R/models_Fk_GAN/model_fk_gan_train.py:374-376.
 *   pose16 (N,16,3) world; quat[4] (w,x,y,z), trans[3], cam9[9] = f(2) c(2) k(3) p(2)  (host arrays)
 *   -> cam3d (N,16,3) optional, proj2d (N,16,2) optional. */
int dhaug_world_to_camera_project(const float* pose16, const float* quat, const float* trans,
                                  const float* cam9, float* cam3d, float* proj2d, int64_t N, void* stream);

/* VJP of the above w.r.t. pose16: grad_cam3d / grad_proj2d (either may be NULL) -> grad_pose16. */
int dhaug_world_to_camera_project_backward(const float* pose16, const float* quat, const float* trans,
                                           const float* cam9, const float* grad_cam3d,
                                           const float* grad_proj2d, float* grad_pose16, int64_t N,
                                           void* stream);

/* camera -> world with per-sample quaternion/translation (N,4),(N,3):
 * GAN_torch_camera_to_world_batch R/common/camera.py:53-59. */
int dhaug_camera_to_world(const float* cam3d, const float* quat, const float* trans, float* world,
                          int64_t N, void* stream);

/* Real-data side of the augmentation API ("next" row N3).
 * dhaug_bone_length_swap: random_bl_aug of R/function_aug/dataloader_update.py:18-40 -- every bone keeps its direction
 * and takes the length new_len[k] (N,15 in PoseAug bone order: (0,1)(1,2)(2,3)(0,4)(4,5)(5,6)(0,7)(7,8)(8,9)(8,10)
 * (10,11)(11,12)(8,13)(13,14)(14,15), R/utils/gan_utils.py:90-138); the pose is rebuilt from the root down.
 * dhaug_project_to_2d: project_to_2d (R/common/camera.py:62-94) of camera-space poses with per-sample intrinsics
 * cam9 (N,9) on the device, as called at dataloader_update.py:69. */
int dhaug_bone_length_swap(const float* pose16, const float* new_len, float* out, int64_t N, void* stream);
int dhaug_project_to_2d(const float* cam3d, const float* cam9, float* proj2d, int64_t N, void* stream);

/* Root-centre and/or left/right flip of (N,16,C) poses, C in {2,3}:
 * x - x[:, :1] (R/models_Fk_GAN/model_fk_gan_train.py:295,312) and the flip of :320-331
 * (negate coordinate 0, swap joints [4,5,6,10,11,12] <-> [1,2,3,13,14,15]). */
int dhaug_center_flip(const float* in, float* out, int64_t N, int C, int center, int flip, void* stream);
/* transpose (VJP) of the linear map above */
int dhaug_center_flip_backward(const float* grad_out, float* grad_in, int64_t N, int C, int center, int flip,
                               void* stream);

/* Clip gather of the video loader: GAN_video_ChunkedGenerator.next_epoch (R/models_Fk_GAN/video_mode_operate.py:126-183) for
 * nrec records (seq, start, end, flip) taken from a device array: for record i and output frame f < frames = end - start + 2*pad,
 *   src = seq_offset[seq] + clamp(start - pad - causal_shift + f, 0, seq_len[seq] - 1)   (== the slice + np.pad 'edge');
 * flip: x -> -x and joint j <- joint perm[j] (perm3d for 3D, perm2d for 2D), camera columns 2 and 7 negated.
 *   seq3d (total_frames,16,3), seq2d (total_frames,16,2): the sequences concatenated; cams (S, cam_w); seq_offset (S) int64 and
 *   seq_len (S) int32: first row and length (>= 1) of each sequence; records (nrec,4) int32, every seq < S (not checked: the
 *   caller builds them) -> out3d (nrec,frames,16,3), out2d (nrec,frames,16,2), out_cam (nrec,cam_w), every element written.
 *   perm3d / perm2d: HOST arrays of 16 entries, read during the call; each a permutation of 0..15 (DHAUG_EINVAL otherwise),
 *   NULL = identity.
 * seq3d/out3d and cams/out_cam may be NULL together (the reference's poses_3d / cameras = None).  seq2d, seq3d, out2d, out3d
 * and records 16-byte aligned (DHAUG_EALIGN); nrec * frames < 2^31 / 12 (DHAUG_EUNSUPPORTED).  Data movement only: the output
 * is the reference's float64 batch cast to fp32, bit for bit. */
int dhaug_clip_gather(const float* seq3d, const float* seq2d, const float* cams, int cam_w,
                      const int64_t* seq_offset, const int32_t* seq_len, const int32_t* records, int64_t nrec,
                      int frames, int pad, int causal_shift, const int8_t* perm3d, const int8_t* perm2d,
                      float* out3d, float* out2d, float* out_cam, void* stream);

/* Clip gather with a window of its own for the 3D and the 2D frames: the batches of ChunkedGenerator.next_epoch and
 * UnchunkedGenerator.next_epoch (R/models_Fk_GAN/video_mode_operate.py:272-347, :381-406), whose 3D target is the chunk's frames
 * and whose 2D input is the padded, shifted window.  For record i = (seq, start, end, flip):
 *   out3d[i, f] = seq3d[seq_offset[seq] + clamp(start - shift3 + f, 0, seq_len[seq] - 1)]   f < frames3
 *   out2d[i, f] = seq2d[seq_offset[seq] + clamp(start - shift2 + f, 0, seq_len[seq] - 1)]   f < frames2
 * with the record's flip and the camera row as in dhaug_clip_gather.  ChunkedGenerator: (frames3, shift3) = (chunk_length, 0),
 * (frames2, shift2) = (chunk_length + 2 pad, pad + causal_shift); UnchunkedGenerator: records (seq, 0, T, flip), (T, 0) and
 * (T + 2 pad, pad + causal_shift).  frames3 = frames2 and shift3 = shift2 = pad + causal_shift is dhaug_clip_gather, bit for bit.
 *   Read extents: seq3d / seq2d rows seq_offset[seq] .. seq_offset[seq] + seq_len[seq] - 1 of every record's sequence (seq_len >= 1,
 *   seq < S: not checked, the caller builds the records); cams row seq; records rows 0 .. nrec - 1; the record's end is not read.
 *   Outputs (nrec,frames3,16,3), (nrec,frames2,16,2), (nrec,cam_w): every element written.  Pointer pairs, permutations and
 *   alignment as dhaug_clip_gather.
 * DHAUG_EINVAL: nrec < 0, frames3 or frames2 < 1, seq3d / out3d or cams / out_cam not NULL together, cam_w < 1 with cameras, a
 * perm that is not a permutation, (nrec > 0) a NULL seq2d / out2d / seq_offset / seq_len / records.  DHAUG_EUNSUPPORTED:
 * nrec * frames3 or nrec * frames2 >= 2^31 / 12, |shift| >= 2^30.  DHAUG_EALIGN as dhaug_clip_gather.  nrec = 0 launches nothing. */
int dhaug_clip_gather_windows(const float* seq3d, const float* seq2d, const float* cams, int cam_w,
                              const int64_t* seq_offset, const int32_t* seq_len, const int32_t* records, int64_t nrec,
                              int frames3, int shift3, int frames2, int shift2, const int8_t* perm3d, const int8_t* perm2d,
                              float* out3d, float* out2d, float* out_cam, void* stream);

/* dhaug_pair_batch (below) of the clips dhaug_clip_gather_windows would write, in one launch straight from the sequences: what one
 * iteration of video_mode_train_posenet (R/models_Fk_GAN/video_mode_operate.py:532-648) reads.  With (p3, p2) = the (out3d, out2d)
 * of dhaug_clip_gather_windows for the same records, windows and permutations, each optional output, every element written:
 *     tgt (nrec,frames3,16,3) = p3 - p3[..., :1, :] per frame;  inp (nrec,frames2,16,2) = p2;
 *     flip != 0:      tgt_flip, inp_flip = the H36M left/right flip of dhaug_center_flip applied to tgt / inp;
 *     playback != 0:  inp_back = inp with the frames reversed, inp_flip_back = the same of inp_flip.
 * Per output frame: the source index is clamped, the record's flip (perm3d / perm2d, the loader's augment) applied, then the
 * training flip, then the frame reversal.  One fp32 subtraction, otherwise copies and signs: equal to
 * dhaug_pair_batch(dhaug_clip_gather_windows(...)) bit for bit.
 *   Read extents and record contract as dhaug_clip_gather_windows (no cameras).  seq3d may be NULL when neither tgt nor tgt_flip
 *   is asked for, seq2d when no inp* is.
 * DHAUG_EINVAL: nrec < 0, frames3 or frames2 < 1, no output at all, an output whose flag is off, a NULL seq3d / seq2d whose
 * outputs are asked for, a perm that is not a permutation, (nrec > 0) a NULL seq_offset / seq_len / records.
 * DHAUG_EUNSUPPORTED: nrec * frames3 or nrec * frames2 >= 2^31 / 12, |shift| >= 2^30.  DHAUG_EALIGN: a float pointer or records
 * not 16-byte, seq_offset not 8-byte, seq_len not 4-byte aligned.  nrec = 0 launches nothing. */
int dhaug_clip_pair_batch(const float* seq3d, const float* seq2d, const int64_t* seq_offset, const int32_t* seq_len,
                          const int32_t* records, int64_t nrec, int frames3, int shift3, int frames2, int shift2,
                          const int8_t* perm3d, const int8_t* perm2d, int flip, int playback, float* tgt, float* inp,
                          float* tgt_flip, float* inp_flip, float* inp_back, float* inp_flip_back, void* stream);

/* Posenet evaluation metrics of P poses, pred / target (P,16,3) fp32, both 16-byte aligned (DHAUG_EALIGN): mpjpe, p_mpjpe,
 * compute_PCK and compute_AUC of R/utils/loss.py (:8-14, :123-164, :192-225) as evaluate (R/function_aug/model_pos_eval.py:16-92)
 * and video_mode_evaluate (R/models_Fk_GAN/video_mode_operate.py:769-876) call them.
 *   center != 0: both poses root-centred first, x - x[:, :1] in fp32 (what evaluate does; the loss functions do not).
 *   joint error e_j = sqrt((dx*dx + dy*dy) + dz*dz) in fp32, d = pred - target, no contraction, correctly rounded sqrt:
 *     numpy's value in compute_PCK bit for bit.  Joint j is a true positive at threshold k if fl32(e_j * 1000) < thresholds[k]
 *     (compared exactly against the fp64 threshold), and then counts multiplicity[j] times.
 *   P-MPJPE of a pose: the mean over its joints of |a * Q (pred_j - muY) + muX - target_j| after the optimal similarity
 *     alignment (the reference's sign-fixed SVD: proper rotation, scale a = (s1 + s2 + sign * s3) * |X0| / |Y0|), in fp64.
 *     NaN where |X0| or |Y0| is 0 (the reference's 0 / 0).
 *   mpjpe_out, pmpjpe_out: optional fp32 (P,) per-pose MPJPE / P-MPJPE (meters, like the inputs), every element written.
 *   totals: optional device dhaug_eval_totals, ACCUMULATED into (the caller zeroes it): sum_err += sum of all e_j (fp64),
 *     sum_pmpjpe += sum of the per-pose P-MPJPE (fp64), poses += P, tp[k] += true positives at threshold k.  Deterministic:
 *     per-workgroup partials in a fixed order, no atomics; the same call sequence gives bit-identical totals.
 *   workspace: device, DHAUG_EVAL_WORKSPACE_BYTES, 8-byte aligned, needed with totals (NULL allowed without); one call at a
 *     time per workspace (stream order).
 *   thresholds: HOST array of nthr doubles, multiplicity: HOST array of 16 ints (NULL = all 1), both read during the call.
 * DHAUG_EINVAL: P < 0, nthr < 0 or > DHAUG_EVAL_MAX_THRESHOLDS, thresholds NULL with nthr > 0, a multiplicity outside
 * [0, DHAUG_EVAL_MAX_MULTIPLICITY], no output at all, totals without a workspace, or (P > 0) a NULL pred / target.
 * DHAUG_EUNSUPPORTED: P >= 2^31.  Two launches (metrics, then the one-wave reduction when totals is given). */
#define DHAUG_EVAL_MAX_THRESHOLDS 32
#define DHAUG_EVAL_MAX_MULTIPLICITY 1024
#define DHAUG_EVAL_WORKSPACE_BYTES (2048 * (3 + DHAUG_EVAL_MAX_THRESHOLDS) * 8)
typedef struct dhaug_eval_totals {
    double sum_err;
    double sum_pmpjpe;
    int64_t poses;
    int64_t tp[DHAUG_EVAL_MAX_THRESHOLDS];
} dhaug_eval_totals;
int dhaug_pose_metrics(const float* pred, const float* target, int64_t P, int center, const double* thresholds, int nthr,
                       const int32_t* multiplicity, float* mpjpe_out, float* pmpjpe_out, void* totals, void* workspace,
                       void* stream);

/* The detailed pose errors of R/utils/loss.py: mpjpe_byjoint :17-23, weighted_mpjpe :26-32, n_mpjpe :167-177 and
 * mean_velocity_error :180-189 (numpy).  Both entries: fp32 inputs, 16-byte aligned (DHAUG_EALIGN); center != 0 subtracts the
 * first joint of every group of 16 joints in fp32, as dhaug_pose_metrics does; every difference, square, square root and sum
 * after that in fp64 from the fp32 values.  Sums are ACCUMULATED into caller-zeroed device doubles.  Deterministic: per-workgroup
 * fp64 partials in the workspace, added in a fixed order by a second launch, no atomics; the same call sequence gives the same
 * bits.  workspace: device, 8-byte aligned, one call at a time per workspace (stream order).
 *
 * dhaug_pose_column_errors: pred / target (rows, cols, 3), cols a multiple of 4 and <= DHAUG_COLERR_MAX_COLS (16 joints x 243
 *   frames).  With e[r,c] = |pred[r,c] - target[r,c]|:
 *     col_sums: optional device double[cols], col_sums[c] += sum over r of e[r,c]  (mpjpe_byjoint = col_sums / rows);
 *     vel_sum:  optional device double[1], += sum over r < rows - 1 and c of
 *               |(pred[r+1,c] - pred[r,c]) - (target[r+1,c] - target[r,c])|  (mean_velocity_error = vel_sum / ((rows - 1) cols));
 *               rows = 1 has no such pair and leaves it untouched.
 *   A workgroup owns a slab of consecutive rows and walks it downwards; the partition into slabs is a function of (rows, cols)
 *   only: with RG = max(1, 1024 / cols) rows per step (1 for cols > 1024) and CC = ceil(cols / 1024) workgroups per row,
 *   at most DHAUG_COLERR_MAX_BLOCKS / CC slabs of at least DHAUG_COLERR_MIN_STEPS steps.  workspace: DHAUG_COLERR_WORKSPACE_BYTES.
 *   DHAUG_EINVAL: rows or cols < 0, neither col_sums nor vel_sum, NULL workspace, center != 0 with cols % 16 != 0, or (rows, cols
 *   > 0) a NULL pred / target.  DHAUG_EUNSUPPORTED: cols > DHAUG_COLERR_MAX_COLS, cols % 4 != 0, rows >= 2^31.  DHAUG_EALIGN also:
 *   col_sums, vel_sum or workspace not 8-byte aligned.  rows = 0 or cols = 0 is a no-op.
 *
 * dhaug_pose_scaled_errors: pred / target P poses of (16, 3).  sums: device double[2]:
 *     sums[0] += sum over poses p and joints j of |s_p pred_pj - target_pj|, s_p = (sum_j target_pj . pred_pj) / (sum_j pred_pj .
 *               pred_pj) in fp64 (n_mpjpe = sums[0] / (16 P)); an all-zero predicted pose gives 0 / 0 = NaN, as the reference;
 *     sums[1] += sum over p, j of w e_pj, e_pj = |pred_pj - target_pj| (weighted_mpjpe = sums[1] / (16 P)): w optional fp32, one
 *               value per joint (w_per_joint != 0: P x 16 values, 16-byte aligned) or per pose (P values, 4-byte aligned), any
 *               sign; with w == NULL sums[1] is untouched.
 *   workspace: DHAUG_SCALEDERR_WORKSPACE_BYTES.
 *   DHAUG_EINVAL: P < 0, NULL sums / workspace, (P > 0) a NULL pred / target.  DHAUG_EUNSUPPORTED: P >= 2^31.  DHAUG_EALIGN also:
 *   sums or workspace not 8-byte aligned.  P = 0 is a no-op.
 * Two launches each (errors, then the reduction of the partials). */
#define DHAUG_COLERR_MAX_COLS (16 * 243)
#define DHAUG_COLERR_MAX_BLOCKS 1024
#define DHAUG_COLERR_MIN_STEPS 4
#define DHAUG_COLERR_WORKSPACE_BYTES ((DHAUG_COLERR_MAX_BLOCKS + DHAUG_COLERR_MAX_BLOCKS * 1024) * 8)
#define DHAUG_SCALEDERR_MAX_BLOCKS 2048
#define DHAUG_SCALEDERR_WORKSPACE_BYTES (DHAUG_SCALEDERR_MAX_BLOCKS * 2 * 8)
int dhaug_pose_column_errors(const float* pred, const float* target, int64_t rows, int64_t cols, int center, double* col_sums,
                             double* vel_sum, void* workspace, void* stream);
int dhaug_pose_scaled_errors(const float* pred, const float* target, int64_t P, int center, const float* w, int w_per_joint,
                             double* sums, void* workspace, void* stream);

/* Posenet training: everything around the posenet call of train_posenet (R/function_aug/model_pos_train.py:13-83),
 * video_mode_train_posenet and GAN_dataSet_video_mode_train_posenet (R/models_Fk_GAN/video_mode_operate.py:532-765).
 *
 * dhaug_pair_batch: the tensors one training iteration consumes, in one launch.  p3 (M,F3,16,3), p2 (M,F2,16,2) fp32 (the
 *   reference's clips carry F2 = receptive field frames of 2D and F3 = 1 or F2 frames of 3D); idx: n int64 DEVICE row indices
 *   into the M rows (not checked: the caller's responsibility), NULL = rows 0..n-1 (then n <= M).  Outputs, each optional, every
 *   element of a given output written:
 *     tgt (n,F3,16,3) = x - x[..., :1, :] per frame;  inp (n,F2,16,2) = the rows as they are;
 *     flip != 0:      tgt_flip, inp_flip = the flip of dhaug_center_flip applied to tgt / inp;
 *     playback != 0:  inp_back = inp with the frames reversed (torch.flip(..., dims=[1])), inp_flip_back = the same of inp_flip.
 *   Data movement, one fp32 subtraction and a sign flip: equal to the torch expressions of the reference bit for bit.
 *   DHAUG_EINVAL: n, M < 0, F3 or F2 < 1, no output at all, an output whose flag is off, a NULL p3 / p2 whose outputs are asked for,
 *   n > M without idx.  All float pointers 16-byte, idx 8-byte aligned (DHAUG_EALIGN); n * max(F3, F2) < 2^31 / 48
 *   (DHAUG_EUNSUPPORTED).  n = 0 is a no-op.
 *
 * dhaug_pose_mse: nn.MSELoss(reduction='mean') forward and backward of numel fp32 elements, two launches.
 *   grad (numel) = fl32(pred - tgt) * fl32(2 / numel), every element written; *loss (device) = the mean of (pred - tgt)^2,
 *   accumulated in fp64 from exact differences and rounded to fp32 once; meter (optional, device dhaug_loss_meter, ACCUMULATED
 *   into): sum_loss_x_poses += (double)*loss * poses, poses += poses, steps += 1 -- AverageMeter.update(loss.item(), poses)
 *   without the host.  workspace: device, DHAUG_POSETRAIN_WORKSPACE_BYTES, 8-byte aligned; one call at a time per workspace
 *   (stream order).  Per-workgroup partials added in a fixed order, no atomics: the same call sequence gives the same bits.
 *   DHAUG_EINVAL: numel or poses < 0, NULL grad / loss / workspace, (numel > 0) NULL pred / tgt.  numel = 0 is a no-op.
 *
 * dhaug_pose_mpjpe: mpjpe of R/utils/loss.py:8-14, torch.mean(torch.norm(pred - tgt, dim=-1)), forward and backward of joints rows
 *   of 3 contiguous fp32 values, the same two launches.  Per joint d = pred - tgt and e = sqrt(dx^2 + dy^2 + dz^2) in fp64 (the
 *   difference is exact); grad (joints x 3) = fl32(d / (e * joints)), rounded once, and exactly 0 in all three components where
 *   e == 0 (torch's subgradient there); every element written.  *loss = fl32(sum of e / joints), the sum in fp64 in a fixed order;
 *   meter, workspace, reproducibility and the one-call-per-workspace rule as dhaug_pose_mse.  pred, tgt, grad: 4-byte aligned;
 *   16-byte aligned bases take the float4 path (four joints per lane), others and the joints % 4 tail a scalar one -- the same
 *   values.  A NaN input gives a NaN loss and a NaN gradient for that joint only.  NOT reproduced from the reference's fp32
 *   arithmetic: the overflow of its squares (|d| >~ 1.8e19 gives an inf loss there) and the zero gradient it returns for a distance
 *   too small for fp32 squares (|d| <~ 1e-23: here the true unit vector over joints).
 *   DHAUG_EINVAL: joints or poses < 0, NULL grad / loss / workspace, (joints > 0) NULL pred / tgt; DHAUG_EALIGN: meter or workspace
 *   not 8-byte aligned.  joints = 0 is a no-op.
 *
 * dhaug_grad_sumsq + dhaug_adam_clip_step: nn.utils.clip_grad_norm_(params, max_norm) (error_if_nonfinite=False) followed by
 *   torch.optim.Adam.step() on flat fp32 vectors of n elements, two launches.
 *   dhaug_grad_sumsq writes per-workgroup fp64 partial sums of (fl32(grad[i] * grad_scale))^2 into workspace (a partition fixed by
 *   n and grad's alignment) and, when step_counter is given, advances that device int by one (the Adam launch reads it).
 *   dhaug_adam_clip_step (same n, grad_scale and workspace): every workgroup adds the partials in index order,
 *   norm = fl32(sqrt(sum)), coef = min(1, max_norm / (norm + 1e-6)) in fp32 (a NaN stays a NaN), and dhaug_adam_step_dev's
 *   arithmetic runs with the gradient (grad[i] * grad_scale) * coef; *step_dev >= 1 is the step count.  norm_out: optional device
 *   float, what clip_grad_norm_ returns.  max_norm = +inf: no clipping.  With coef == 1 the parameters and both moments are
 *   bit-identical to dhaug_adam_step_dev.  A NaN gradient makes every parameter NaN; an inf gradient makes coef 0, that element's
 *   update NaN and the others' gradient 0 -- as torch.
 *   DHAUG_EINVAL: n < 0, NULL workspace / step_dev, max_norm <= 0 or NaN, (n > 0) a NULL vector.  n = 0 is a no-op. */
#define DHAUG_GRAD_SUMSQ_MAX_PARTIALS 1024
#define DHAUG_POSETRAIN_WORKSPACE_BYTES (2048 * 8)
typedef struct dhaug_loss_meter {
    double sum_loss_x_poses;
    int64_t poses;
    int64_t steps;
} dhaug_loss_meter;
int dhaug_pair_batch(const float* p3, const float* p2, int64_t M, int F3, int F2, const int64_t* idx, int64_t n, int flip,
                     int playback, float* tgt, float* inp, float* tgt_flip, float* inp_flip, float* inp_back,
                     float* inp_flip_back, void* stream);
int dhaug_pose_mse(const float* pred, const float* tgt, int64_t numel, int64_t poses, float* grad, float* loss, void* meter,
                   void* workspace, void* stream);
int dhaug_pose_mpjpe(const float* pred, const float* tgt, int64_t joints, int64_t poses, float* grad, float* loss, void* meter,
                     void* workspace, void* stream);
int dhaug_grad_sumsq(const float* grad, int64_t n, float grad_scale, void* workspace, int* step_counter, void* stream);
int dhaug_adam_clip_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                         float beta2, float eps, const int* step_dev, float grad_scale, float max_norm, const void* workspace,
                         float* norm_out, void* stream);
/* dhaug_adam_clip_step_lr: dhaug_adam_clip_step with the learning rate in device memory, for a launch that is captured once and
 *   replayed under a schedule.  lr_dev: one device float (4-byte aligned), read by every workgroup; every other argument, check and
 *   code is dhaug_adam_clip_step's, and for *lr_dev == lr the parameters, both moments and norm_out are its bits (one kernel,
 *   instantiated for the two sources of lr).  DHAUG_EINVAL in addition: NULL lr_dev (checked before n = 0 returns). */
int dhaug_adam_clip_step_lr(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr_dev,
                            float beta1, float beta2, float eps, const int* step_dev, float grad_scale, float max_norm,
                            const void* workspace, float* norm_out, void* stream);
/* *cell += value on a device uint64 (8-byte aligned: DHAUG_EALIGN otherwise; NULL: DHAUG_EINVAL), a one-workgroup launch in stream
 *   order like dhaug_counter_add: the base of the device dropout stream (dhaug_bn_act_forward_dr) is advanced with it once per step. */
int dhaug_u64_add(uint64_t* cell, uint64_t value, void* stream);

/* The other criteria of R/utils/loss.py, forward and backward like dhaug_pose_mpjpe (csrc/dhaug_pose_criteria.hip): n_mpjpe
 * :167-177, weighted_mpjpe :26-32 and the backward of mpjpe_byjoint :17-23.  fp32 in and out; every difference, square, square
 * root, scale and sum in fp64 from the fp32 values; each gradient element rounded to fp32 once; every element of grad written.
 *
 * dhaug_pose_nmpjpe: P poses of (16, 3), two launches.  Per pose, in fp64: pp = sum p.p, tp = sum t.p, s = tp / pp (the
 *   reference's two means over the joints cancel), r_j = s p_j - t_j, e_j = |r_j|, u_j = r_j / e_j and exactly 0 where e_j == 0,
 *   a = sum_j u_j.p_j.  With J = 16 P:
 *     grad_k = fl32((s u_k + a (t_k - 2 s p_k) / pp) / J)   -- torch's autograd of the reference's expression;
 *     *loss  = fl32(sum of e / J), per-workgroup fp64 partials added in index order by a one-wave second launch.
 *   Four lanes per pose, each holding four joints in registers; 64 poses per workgroup in a grid-stride loop; the pose's sums meet
 *   in two-level butterflies over its four lanes: every input element is read once.  pred, tgt, grad: 4-byte aligned; bases on a
 *   16-byte boundary take the float4 path, others a scalar one with the same values.  A pose whose pp is 0 gives a NaN loss and 48
 *   NaN gradient values for that pose only, as the reference; a NaN input stays inside its pose's 48 gradient values (and reaches
 *   the loss).  A pose the prediction fits exactly up to scale (every e_j == 0) gets an all-zero gradient.
 *   meter (optional, ACCUMULATED into with `poses`, which is the caller's count and need not be P), workspace
 *   (DHAUG_POSETRAIN_WORKSPACE_BYTES), reproducibility and the one-call-per-workspace rule as dhaug_pose_mse.
 *   DHAUG_EINVAL: P or poses < 0, NULL grad / loss / workspace, (P > 0) NULL pred / tgt; DHAUG_EUNSUPPORTED: P >= 2^31;
 *   DHAUG_EALIGN: meter or workspace not 8-byte aligned.  P = 0 is a no-op.
 *
 * dhaug_pose_wmpjpe: mean(w |pred - tgt|) of P poses of (16, 3), the same layout, launches, meter, workspace and codes.  w_mode:
 *     DHAUG_WMPJPE_PER_POSE  (1) one fp32 weight per pose, P values, 4-byte aligned;
 *     DHAUG_WMPJPE_PER_JOINT (2) one per pose and joint, P x 16 values, 16-byte aligned;
 *     DHAUG_WMPJPE_SHARED    (3) one per joint shared by all poses, 16 values, 4-byte aligned.
 *   Weights of any sign.  With d = pred - tgt, e = |d|: grad = fl32(w d / (e J)), exactly 0 where e == 0; *loss = fl32(sum of
 *   w e / J).  A NaN input gives a NaN loss and a NaN gradient for that joint only.
 *   DHAUG_EINVAL in addition: NULL w or any other w_mode (checked before P = 0 returns).
 *
 * dhaug_pose_byjoint_backward: the backward of mpjpe_byjoint for (rows, cols, 3) joints, one launch.  cot: device fp32[cols], the
 *   cotangent of the per-column means; grad[r, c] = fl32(cot[c] d / (e rows)), exactly 0 where e == 0.  All pointers 4-byte
 *   aligned; four joints per lane on 16-byte aligned pred / tgt / grad, a scalar path otherwise and for the rows cols % 4 tail.
 *   (The forward value is dhaug_pose_column_errors'.)  DHAUG_EINVAL: rows or cols < 0, (rows, cols > 0) a NULL pointer;
 *   DHAUG_EUNSUPPORTED: rows or cols >= 2^31.  rows = 0 or cols = 0 is a no-op. */
#define DHAUG_WMPJPE_PER_POSE 1
#define DHAUG_WMPJPE_PER_JOINT 2
#define DHAUG_WMPJPE_SHARED 3
int dhaug_pose_nmpjpe(const float* pred, const float* tgt, int64_t P, int64_t poses, float* grad, float* loss, void* meter,
                      void* workspace, void* stream);
int dhaug_pose_wmpjpe(const float* pred, const float* tgt, int64_t P, const float* w, int w_mode, int64_t poses, float* grad,
                      float* loss, void* meter, void* workspace, void* stream);
int dhaug_pose_byjoint_backward(const float* pred, const float* tgt, int64_t rows, int64_t cols, const float* cot, float* grad,
                                void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Dense layers: bf16 MFMA GEMM with fused epilogue
 * ---------------------------------------------------------------------------------------------------- */

/* C[M,N] = act( A[M,K] * B[N,K]^T + bias[N] + residual[M,N] )      (v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16, fp32 acc)
 * A, B bf16 row-major, contraction dimension contiguous in both (nn.Linear weight layout [out,in]).
 * Replaces nn.Linear + ReLU/LeakyReLU + residual add of myResNet (R/models_Fk_GAN/special_operate.py:490-510)
 * and the Linear stacks of R/models_Fk_GAN/Fk_generator.py:95-103, Fk_discriminator.py:156-178,243-249.
 *   K % 16 == 0 (operands zero-padded by their producers); lda, ldb, ld_res, ldc_* in elements, % 8 == 0.
 *   bias     : fp32 [N] or NULL.
 *   residual : bf16 (M, ld_res) or NULL, added before the activation.
 *   residual_f32 : fp32 (M, ld_res_f32) or NULL, same role (fp32-grade "bf16x3" path).
 *   c_bf16   : optional bf16 output (M, ldc_bf16); columns [N, n_pad_zero) are written as 0 so the result
 *              can feed the next GEMM as a zero-padded operand.
 *   c_f32    : optional fp32 output (M, ldc_f32).
 * At least one output must be given.
 * READ EXTENT (every dhaug_gemm_bf16* entry point, dhaug_gemm_bf16_group members included): each of the M rows of A and of the N
 * rows of B is read over EXACTLY K columns -- elements [r * ld, r * ld + K) of row r, nothing beyond them (no kernel reads past
 * column K; the K tail of a tile is clamped or zero-sourced) -- and the rows of residual / dmask over N columns.  A caller that
 * passes a K wider than the data of a row (a 1000-column block of a wider buffer contracted with K = 1008 against zero weight
 * columns) must therefore own all K columns of the LAST row too, and they must hold finite values: 0 * NaN = NaN.  The Python
 * host layer gives such buffers a guard row (critic_step._Math.empty_blocks, gen_step); tests/test_gpu_graphs.py::
 * test_whole_iterations_read_no_unwritten_memory and tests/test_gpu_gemm_p8.py::test_p8_reads_nothing_beyond_k hold both sides.
 * Kernels: 256-wide layers of whole 32-row tiles -> gemm_nt256s; K <= 256 -> the weight-stationary kernel; wide layers with tiles
 * enough for the card (and grouped members of >= 1024 rows) -> the 256 x 256 x 64 ping-pong kernel (csrc/dhaug_gemm_p8.hip);
 * otherwise 64 x 64 / 128 x 128 pipelined tiles.  All sum k ascending into one fp32 accumulator per output. */
int dhaug_gemm_bf16(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb,
                    const float* bias, const uint16_t* residual, int64_t ld_res,
                    const float* residual_f32, int64_t ld_res_f32,
                    uint16_t* c_bf16, int64_t ldc_bf16, int64_t n_pad_zero,
                    float* c_f32, int64_t ldc_f32,
                    int64_t M, int64_t N, int64_t K, int act, float slope, void* stream);

/* The split-operand ("bf16x3" / "bf16x6") form of the same step: fp32 result, fp32 residual, and the mask read from the producing
 * layer's fp32 activation: c_f32 = (A B^T + residual_f32) * dmask_act'(dmask), dmask (M, >= N) fp32 (ReLU / LeakyReLU only).  A, B:
 * the operands dhaug_split_bf16 makes (K = terms * padded width).  One launch instead of the GEMM + dhaug_act_backward_f32. */
int dhaug_gemm_bf16_dmask_f32(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const float* residual_f32, int64_t ld_res_f32,
                              const float* dmask, int64_t ld_dmask, int dmask_act, float dmask_slope, float* c_f32, int64_t ldc_f32,
                              int64_t M, int64_t N, int64_t K, void* stream);

/* Input gradient of a layer whose input came out of an activation, in one pass:
 *   c_bf16[M,N] = ( A[M,K] * B[N,K]^T + residual[M,N] ) * act'(dmask[M,N])      act'(y) = y > 0 ? 1 : (ReLU 0 | LeakyReLU slope)
 * i.e. LinearT followed by the activation backward of the producing layer (the `loss.backward()` of
 * R/models_Fk_GAN/special_operate.py:490-510 myResNet: gh * relu'(h)); dmask_act = DHAUG_ACT_NONE gives the plain
 * product.  256-wide layers apply the mask in the GEMM epilogue, other shapes run the GEMM and
 * dhaug_act_backward_bf16 in place. */
int dhaug_gemm_bf16_dmask(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const uint16_t* residual,
                          int64_t ld_res, const uint16_t* dmask, int64_t ld_dmask, int dmask_act, float dmask_slope,
                          uint16_t* c_bf16, int64_t ldc_bf16, int64_t M, int64_t N, int64_t K, void* stream);

/* Same with columns [N, n_pad_zero) of c_bf16 written as 0 (the result feeds the next GEMM as a zero-padded operand) and
 * any N: every kernel applies the mask in its epilogue. */
int dhaug_gemm_bf16_dmask_pad(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const uint16_t* residual,
                              int64_t ld_res, const uint16_t* dmask, int64_t ld_dmask, int dmask_act, float dmask_slope,
                              uint16_t* c_bf16, int64_t ldc_bf16, int64_t n_pad_zero, int64_t M, int64_t N, int64_t K,
                              void* stream);

/* The 256 -> 256 input-gradient / tangent step with the activation mask as a SIGN-BIT array:
 *   c = (A * B^T + residual) * act'(y),   act'(y) read as one bit per element, (y > 0), from `bits` -- the array a
 * forward-with-save layer leaves beside its image (struct dhaug_mlp_unit.bits: same layout, same 32-row tiles; pass the
 * address of the word of the first row's tile when A starts at a later row, a multiple of 32).  M a multiple of 32,
 * N = K = 256, bf16 in / out.  Same arithmetic as dhaug_gemm_bf16_dmask; the mask costs 32 bytes per row instead of 512. */
int dhaug_gemm_bf16_dbits(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const uint16_t* residual, int64_t ld_res,
                          const uint32_t* bits, int dmask_act, float dmask_slope, uint16_t* c_bf16, int64_t ldc_bf16, int64_t M,
                          void* stream);

/* (A B^T) * act'(mask) for an output of one or two 256-wide column blocks whose masks are sign-bit arrays (bits_lo: columns
 * 0..255, bits_hi: 256..511; N = 256 or 512, K <= 256 one of 16, 32, 48, 64, 112, 128, 256): the input-gradient step through
 * the 3D critic's merge layer, R/models_Fk_GAN/Fk_discriminator.py:192-197 under loss.backward() -- the cotangent of the two
 * concatenated branch outputs, each masked by ITS branch's last ReLU. */
int dhaug_gemm_bf16_dbits_wide(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const uint32_t* bits_lo,
                               const uint32_t* bits_hi, int dmask_act, float dmask_slope, uint16_t* c_bf16, int64_t ldc_bf16,
                               int64_t M, int64_t N, int64_t K, void* stream);

/* The one-workgroup-per-CU (persistent) launches of this library -- the fused programs, the 256-wide layer kernels, the block
 * kernel, the grouped weight gradients -- take at most n workgroups from now on (0 or 256: the whole card); returns the
 * previous value.  Process-wide, read at launch time: set it around the launches of one stream and to the complement around
 * another stream's, and the two chains run side by side on disjoint sets of CUs instead of queueing for the whole card. */
int dhaug_set_workgroup_cap(int n);

/* Non-finite values in the fused INFERENCE programs (dhaug_mlp_forward without save targets, dhaug_mlp_forward_x3).  Default
 * (0): their ReLU is an integer max on the bit pattern -- one instruction in the matrix pipe's shadow -- which lets +NaN pass
 * and turns the matrix pipe's -NaN into 0: a NaN / inf input row or a NaN weight does NOT reach the logit through a ReLU
 * layer (LeakyReLU layers, i.e. the 2D critic, always propagate).  on != 0: every ReLU is applied as max(v, v * 0) in fp32
 * like the forward-with-save unit of the training steps does: a NaN / inf input row gives NaN in ITS logit (no other), NaN
 * weights give NaN logits everywhere -- what R/models_Fk_GAN/Fk_discriminator.py:180-201 does through ATen (inf * 0 = NaN:
 * an inf activation becomes NaN one layer earlier than in the reference, the logit is NaN either way).  Same results for
 * finite values; measured cost on MI355X: bf16 programs +5 % (D3 114 -> 120 us at B = 65 536).  Process-wide, read at launch
 * time; returns the previous value.  The Python package sets it from DHAUG_NAN_PROPAGATION=1 at load. */
int dhaug_set_nan_propagation(int on);

/* Two 256 -> 256 layers of a residual block in one launch (the backward step through myResNet,
 * R/models_Fk_GAN/special_operate.py:490-510 under loss.backward(), and its tangent twin in the gradient penalty's
 * double backward, R/models_Fk_GAN/Fk_discriminator.py:205-231):
 *     Y1 = (X W1^T) * act'(bits1)        Y2 = (Y1 W2^T + X) * act'(bits2)
 * X, Y1, Y2: bf16 (M, ld >= 256), M a multiple of 32, three distinct buffers; W1, W2: bf16 (256, ld >= 256) with the
 * contraction along the row (the operand dhaug_gemm_bf16_dbits takes as B); bits1, bits2: sign-bit arrays of the layers'
 * saved activations (struct dhaug_mlp_unit.bits).  Y1 never leaves LDS between the layers and X is read once: 300 MB
 * per 3 x 65 536-row block instead of the 500 MB of two dhaug_gemm_bf16_dbits launches. */
int dhaug_gemm_block2_bf16(const uint16_t* X, int64_t ldx, const uint16_t* W1, int64_t ldw1, const uint16_t* W2, int64_t ldw2,
                           const uint32_t* bits1, const uint32_t* bits2, int mask_act, float mask_slope,
                           uint16_t* Y1, int64_t ldy1, uint16_t* Y2, int64_t ldy2, int64_t M, void* stream);
/* A chain of such blocks in one launch: block i + 1 takes block i's Y2 as its X (the three myResNet blocks of a branch of the
 * critics, backward: block 3, 2, 1; tangent: 1, 2, 3).  Row tiles are independent and a workgroup keeps its tiles through the
 * chain, so the launch needs no device-wide synchronisation between the blocks.  `blocks`: host array, read during the call. */
#define DHAUG_BLOCK2_MAX 3
typedef struct dhaug_block2 {
    const uint16_t* W1; int64_t ldw1;
    const uint16_t* W2; int64_t ldw2;
    const uint32_t* bits1; const uint32_t* bits2;
    uint16_t* Y1; int64_t ldy1;
    uint16_t* Y2; int64_t ldy2;
} dhaug_block2;
int dhaug_gemm_block2_stack_bf16(const uint16_t* X, int64_t ldx, const dhaug_block2* blocks, int nb, int mask_act, float mask_slope,
                                 int64_t M, void* stream);

/* Weight-gradient GEMM: C[N1,N2] (+)= A[M,N1]^T * B[M,N2], contraction over the batch dimension M
 * (split across workgroups, fp32 atomics into C).  bf16 operands, fp32 result.  `accumulate` != 0 adds
 * into C, otherwise C is overwritten (zeroed by the library on the stream first).  colsum_a (optional, fp32 [N1])
 * receives the column sums of A over M -- the bias gradient of the same layer -- computed on the matrix pipe as
 * A^T * ones by the workgroups that already hold the A tiles (same accumulate / overwrite rule as C).
 * M < 1024 is cut in at most two slices: onto a zeroed C their sum is the same bits in either order, so a short contraction
 * repeats its result run to run; a longer one (three or more atomic addends per element) may differ in the last bits. */
int dhaug_gemm_tn_bf16(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb,
                       float* C, int64_t ldc, float* colsum_a, int64_t M, int64_t N1, int64_t N2, int accumulate,
                       void* stream);
/* Same, with the column sums restricted to rows [0, colsum_rows) of A (colsum_rows == M or a multiple of 128): the
 * explicit critic step contracts real, fake AND interpolated rows in one launch, but only the real / fake rows carry a
 * bias gradient (the gradient penalty has none). */
int dhaug_gemm_tn_bf16_rows(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb,
                            float* C, int64_t ldc, float* colsum_a, int64_t colsum_rows, int64_t M, int64_t N1, int64_t N2,
                            int accumulate, void* stream);

/* n <= 8 independent GEMMs of the same (M, N, K) as ONE launch (64 x 64 tiles, blockIdx.y = member): member i computes what
 * dhaug_gemm_bf16 (dmask == NULL or dmask_act == DHAUG_ACT_NONE) / dhaug_gemm_bf16_dmask_pad compute from the same fields --
 * c = act(A B^T + bias + residual + residual_f32), then * dmask_act'(dmask).  For the branches of a motion critic
 * (R/models_Fk_GAN/Fk_discriminator.py:381-587: four / two stacks of identical layers over different features): a 1 536 x 1000 x 1000
 * layer alone is one and a half waves of the card's workgroup slots behind a launch of its own.  N > 64, K >= 64; everything else
 * as dhaug_gemm_bf16. */
typedef struct dhaug_gemm_desc {
    const uint16_t* A; int64_t lda;
    const uint16_t* B; int64_t ldb;
    const float* bias;
    const uint16_t* residual; int64_t ld_res;
    const float* residual_f32; int64_t ld_res_f32;
    uint16_t* c_bf16; int64_t ldc_bf16; int64_t n_pad_zero;
    float* c_f32; int64_t ldc_f32;
    int64_t M, N, K;
    int32_t act; float slope;
    const uint16_t* dmask; int64_t ld_dmask; int32_t dmask_act; float dmask_slope;
} dhaug_gemm_desc;
int dhaug_gemm_bf16_group(const dhaug_gemm_desc* members, int n, void* stream);

/* The weight / bias gradients of ALL layers of a critic step in one launch (+ one small launch that sums the partial
 * results): layer i computes C[N1,N2] (+)= A[M,N1]^T * B[M,N2] and colsum_a[N1] (+)= column sums of A over rows
 * [0, colsum_rows), M and colsum_rows multiples of 32, operands bf16 with rows readable up to ceil8(N) columns (of every
 * 256-column block).  N1, N2 <= 256, or "wide" (up to 4096: a grid of 256 x 256 blocks, one workgroup each -- for
 * groups that have blocks enough to fill the card without splitting any over the batch: the DenseDim-1000 layers of a video step).
 * A block that ends up with ONE workgroup adds its result into C / colsum_a itself (no partial result, no sum).  One workgroup per CU owns a layer's WHOLE output over its slice of the batch (every operand byte crosses
 * L2 -> LDS once; the 64 x 64-tile kernel behind dhaug_gemm_tn_bf16 re-reads each row four times); the workgroups are dealt
 * out to the layers by what their 32-row stages cost (operand bytes, with a floor for narrow layers), so a step leaves 256
 * partial results in total, not per layer.
 * `layers`: host array (read during the call).  `workspace`: DHAUG_TN_GROUP_WORKSPACE_FLOATS fp32 values owned by the
 * caller, any content (calls sharing it must be ordered on one stream).
 * The outputs of ONE call must be distinct: no two layers may name the same C or the same colsum_a (they are summed
 * concurrently, a one-workgroup block with a plain read-modify-write) -- DHAUG_EINVAL otherwise.  A second contribution
 * to a gradient goes into a second call (stream order is the synchronisation).
 * Replaces the parameter-gradient half of loss.backward() in R/models_Fk_GAN/model_fk_gan_train.py:191-214. */
#define DHAUG_TN_GROUP_MAX 42
#define DHAUG_TN_GROUP_WORKSPACE_FLOATS (256LL * (256 * 256 + 256))
typedef struct dhaug_tn_layer {
    const uint16_t* A; int64_t lda;
    const uint16_t* B; int64_t ldb;
    float* C; int64_t ldc;
    float* colsum_a;            /* optional */
    int64_t colsum_rows;
    int64_t M;
    int32_t N1, N2;
    int32_t accumulate;         /* != 0: add into C / colsum_a, else overwrite */
    int32_t max_workgroups;     /* of layers[0]: the launch uses at most this many workgroups (0: one per CU) -- a launch that
                                   runs beside other kernels leaves them CUs */
    int32_t planes_a, planes_b; /* 0: A / B is an ordinary (M, N) operand.  1 / 2: it is dhaug_split_bf16(x, mode 2, terms 6) seen as
                                   (M / 2, ceil16 N) rows -- the three distinct pieces [hi | mid | lo] of every tensor row -- and the
                                   contraction runs over M = 6 x (tensor rows) VIRTUAL rows, virtual row 6 m + t being piece
                                   (0 0 1 1 0 2)[t] (1: the order of the mode 0 split) or (0 1 0 1 2 0)[t] (2: mode 1) of tensor row m:
                                   the same sum, bit for bit, as over the mode 0 / mode 1 operand seen as (6 x rows, ceil16 N), from half
                                   the bytes (the "bf16x6" weight gradients, autograd_ops._raw_outer).  M % 6 == 0 then. */
} dhaug_tn_layer;
int dhaug_gemm_tn_group_bf16(const dhaug_tn_layer* layers, int n, float* workspace, void* stream);

/* fp32 -> bf16 (round-to-nearest-even) with zero padding: src (rows, cols) ld_src -> dst (rows, ld_dst),
 * columns [cols, pad_cols) zero-filled.  Used to pack weights / inputs as GEMM operands. */
int dhaug_cast_pad_bf16(const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst,
                        int64_t rows, int64_t cols, int64_t pad_cols, void* stream);

/* Same with transposition: src (rows, cols) -> dst (cols, ld_dst) = src^T, columns [rows, pad_cols) zero. */
int dhaug_cast_transpose_bf16(const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst,
                              int64_t rows, int64_t cols, int64_t pad_cols, void* stream);

/* Operand split for fp32-grade products on the bf16 MFMA path (the parity modes "bf16x3" / "bf16x6").
 *   terms 3: x = hi + lo.         mode 0 (activation side) row = [hi|hi|lo],            mode 1 (weight side) [hi|lo|hi]
 *   terms 6: x = hi + mid + lo.   mode 0 row = [hi|hi|mid|mid|hi|lo],                   mode 1 [hi|mid|hi|mid|lo|hi]
 * each segment pad_cols wide (zero padded), so that A' * B'^T sums every product term down to 2^-16 (terms 3) or
 * 2^-24 (terms 6) relative.  dst is (rows, terms*pad_cols) contiguous. */
int dhaug_split_bf16(const float* src, int64_t ld_src, uint16_t* dst, int64_t rows, int64_t cols,
                     int64_t pad_cols, int mode, int terms, void* stream);
/* (terms 6 only) mode 2: the three DISTINCT pieces once, row = [hi|mid|lo] (dst is (rows, 3*pad_cols)): half the bytes of mode 0.  The
 * operand of dhaug_gemm_bf16x6_planes, which reads piece (0 0 1 1 0 2)[s] for K-segment s -- the mode 0 row without its copies. */

/* c_f32[M,N] = act( X W^T + bias + residual_f32 ) * (dmask_f32 > 0 ? 1 : dneg) in the "bf16x6" arithmetic with the activation side as
 * PLANES: A_planes = dhaug_split_bf16(x, mode 2, terms 6) = [hi|mid|lo] of kp columns each (lda >= 3 kp), B = dhaug_split_bf16(W, mode 1,
 * terms 6) (ldb >= 6 kp) with x_order 0; x_order 1: the planes stand for the mode 1 operand and B is the mode 0 split (the backward
 * chain: the cotangent is split once, in the layout the weight gradients contract it in).
 * The same six product terms in the same order as dhaug_gemm_bf16 on the mode 0 / mode 1 operand (K = 6 kp) -- BIT-identical
 * results -- but the split writes 6 instead of 12 bytes per value and the GEMM's re-reads of a piece come from L2 / MALL, not from HBM.
 * kp = 64 * 2^j (a K-tile never straddles two pieces); runs on the 256 x 256 x 64 ping-pong tiles only (csrc/dhaug_gemm_p8.hip): N % 8 == 0,
 * 16-byte aligned bias / residual / mask / output with row pitches % 4 == 0, DHAUG_EUNSUPPORTED otherwise (the caller then splits with
 * mode 0 and calls dhaug_gemm_bf16).  dmask_act DHAUG_ACT_NONE: no mask.
 * x_order 2: A_planes is the ordinary six-segment operand (mode 0, lda >= 6 kp, any kp % 8 == 0 with 6 kp >= 128: a narrow input
 * layer whose RESULT is wanted as planes).  c_planes (optional; ld_planes >= 3 N, % 8 == 0, 16-byte
 * aligned): the result once more as planes [hi|mid|lo] of N columns each -- bit for bit what dhaug_split_bf16(c_f32, mode 2, terms 6,
 * pad_cols N) makes of it, written by the epilogue that holds the values: the next layer's operand without a split launch.  Replaces, with the split, the fp32 layer products of the
 * training passes, R/models_Fk_GAN/model_fk_gan_train.py:177-230. */
int dhaug_gemm_bf16x6_planes(const uint16_t* A_planes, int64_t lda, const uint16_t* B, int64_t ldb, const float* bias,
                             const float* residual_f32, int64_t ld_res_f32, const float* dmask_f32, int64_t ld_dmask_f32, int dmask_act,
                             float dmask_slope, float* c_f32, int64_t ldc_f32, uint16_t* c_planes, int64_t ld_planes, int64_t M, int64_t N,
                             int64_t kp, int x_order, int act, float slope, void* stream);

/* The same split with IEEE-half pieces, x = hi + lo (22 significant bits; three product terms: mode 0 row = [hi|hi|lo], mode 1
 * [hi|lo|hi]; mode 2: the two distinct pieces once, [hi|lo], dst (rows, 2*pad_cols)): the operands of dhaug_gemm_f16x3[_planes].
 * |x| < 65 504. */
int dhaug_split_f16(const float* src, int64_t ld_src, uint16_t* dst, int64_t rows, int64_t cols, int64_t pad_cols, int mode,
                    void* stream);

/* c_f32[M,N] = act( A[M,K] * B[N,K]^T + bias + residual_f32 ) on IEEE-half operands (v_mfma_f32_16x16x32_f16, fp32 accumulate):
 * with A = dhaug_split_f16(x, mode 0) and B = dhaug_split_f16(W, mode 1), K = 3 * padded width, this is the layer
 * x W^T in the "f16x3" arithmetic of the fused parity programs (Whi Xhi + Whi Xlo + Wlo Xhi: logits <= 1e-4 rel of the fp32
 * reference, R/models_Fk_GAN/Fk_discriminator.py:180-201, 253-266, 381-587) at ANY width -- the parity-grade forward at the
 * reference's default DenseDim 1000 (R/function_aug/config.py:101-109), where the fused programs do not apply.  Runs on the
 * 256 x 256 x 64 ping-pong tiles (csrc/dhaug_gemm_p8.hip); takes K >= 128, N % 8 == 0, ldc_f32 % 4 == 0 and 16-byte aligned bias /
 * residual / output, DHAUG_EUNSUPPORTED otherwise (the caller then runs that layer in "bf16x6").  Read extent as dhaug_gemm_bf16. */
int dhaug_gemm_f16x3(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const float* bias, const float* residual_f32,
                     int64_t ld_res_f32, float* c_f32, int64_t ldc_f32, int64_t M, int64_t N, int64_t K, int act, float slope,
                     void* stream);
/* The same layer with the split LEFT OUT of the chain of layers: the activation side may come as the two distinct pieces [hi|lo] of kp
 * columns each (a_planes != 0: A = dhaug_split_f16(x, mode 2), lda >= 2 kp, kp = 64 * 2^j -- DenseDim 1000 is padded to 1 024 --; the
 * kernel reads piece (0 0 1)[s] for K-segment s of B = dhaug_split_f16(W, mode 1, pad kp); a_planes == 0: A is the mode 0 operand,
 * lda >= 3 kp, any kp), and the result may be written once more as such pieces (c_planes, optional: planes_kp >= N columns per piece,
 * any multiple of 8 -- no power of two is asked of the producer, only of the layer that takes the pieces as its a_planes operand --,
 * ld_planes >= 2 planes_kp and % 8 == 0, columns [N, planes_kp) of both pieces zero for EVERY such planes_kp: the launch covers
 * max(N, planes_kp) columns with tiles, so a pad that reaches beyond the last 256-column tile of N is written too; columns beyond
 * 2 planes_kp of a wider row are left alone) -- bit for bit dhaug_split_f16(c_f32, mode 2, pad planes_kp), from the
 * epilogue's registers: the next layer's operand without a split launch (4 instead of 6 bytes per value, read and written once).
 * Same product terms in the same order as dhaug_gemm_f16x3 on the mode 0 operand of the same padded width: identical results.
 * DHAUG_EUNSUPPORTED where the ping-pong kernel does not take the shape. */
int dhaug_gemm_f16x3_planes(const uint16_t* A, int64_t lda, int a_planes, const uint16_t* B, int64_t ldb, const float* bias,
                            const float* residual_f32, int64_t ld_res_f32, float* c_f32, int64_t ldc_f32, uint16_t* c_planes, int64_t ld_planes,
                            int64_t planes_kp, int64_t M, int64_t N, int64_t kp, int act, float slope, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Fused multi-layer forward (one launch per network; activations stay in LDS)
 * ---------------------------------------------------------------------------------------------------- */

/* Weight fragments in MFMA A-operand order for dhaug_mlp_forward:
 *   dst[((slice*ksteps + ks)*64 + lane)*8 + j] = bf16( W[32*slice + (lane&31)][k0 + 16*ks + 8*(lane>>5) + j] )
 * (0 outside N x K), ksteps = 4*ceil(K/64) <= 16 (whole 64-wide chunks), slice = 0..7 (always 8 slices = 256
 * feature rows, zero beyond N): dst holds 8 * ksteps * 512 bf16.  W is the fp32 nn.Linear weight
 * [N, ldw]; (k0, K) selects a column range (layers fed by a concatenation take one block per source). */
int dhaug_pack_wfrag(const float* W, int64_t ldw, uint16_t* dst, int64_t N, int64_t K, int64_t k0, void* stream);

/* One unit of a fused network program.  Three LDS activation buffers exist per 128-row batch tile:
 * ids 0 and 1 hold up to 256 bf16 columns, id 2 up to 128. */
#define DHAUG_MLP_LOAD_F32    0   /* global fp32 (M, ld) columns [0, cols) -> buffer dst (rounded to bf16)          */
#define DHAUG_MLP_LOAD_BF16   1   /* global bf16 (M, ld) columns [0, cols) -> buffer dst                              */
#define DHAUG_MLP_STORE_BF16  2   /* buffer src columns [0, cols) -> global bf16 (M, ld)                              */
#define DHAUG_MLP_GEMM        3   /* one layer: dst = act(W * src [+ W2 * src2] + bias + res)                          */
/* Where a GEMM unit rounds.  Products of bf16 operands, the fp32 bias and the residual (a bf16 value, added as 1.0 * res on the
 * matrix unit) are accumulated in fp32.  The activation is applied to that fp32 value (LeakyReLU: max(v, v * slope) in fp32; ReLU
 * may be taken after the rounding, which gives the same bf16 value), and the result is rounded ONCE, to nearest even, to bf16 when
 * it goes to an LDS buffer -- whence a later GEMM, a STORE_BF16 or a `save` target takes it unchanged -- or into the dot product
 * of a DOT_OUT unit: that epilogue rounds and activates the features exactly as it would have stored them, multiplies them by w2
 * in fp32 (fmaf) and adds the folded bias.  An OUT_F32 result is not rounded: act(.) leaves as the fp32 value the accumulator
 * held; such a unit takes no residual (res >= 0: DHAUG_EINVAL).  A LOAD_F32 rounds its input to bf16 the same way.  With data for
 * which every partial sum is an fp32 value (tests/mlp_unit_util.py) a program's output is therefore one definite bit pattern,
 * whatever route its units take.
 * A unit writes whole 32-feature slices: columns [0, 32 * ceil(n / 32)) of dst, the ones beyond n as act(res) (zero weights and
 * bias).  What the columns beyond hold afterwards is unspecified (a run of full-width layers writes all 256, a layer on its own
 * leaves them as they were); a consumer reads whole 64-column chunks under zero weights there, so they must hold finite values.
 * For the run planner a layer with n > 224 (eight slices) counts as full width: its consumer is handed ksteps = 16, with zero
 * weight columns beyond n.  A second source starts on a chunk boundary of the first (ksteps % 4 == 0) and the two take 1 + 1,
 * 2 + 2 or 4 + 4 chunks: fewer columns in the second source are loaded and packed as whole chunks of the first's count. */
#define DHAUG_MLP_LOAD_KCS    5   /* dhaug_mlp_forward_x3 only: global fp32 poses (M, ld >= 48) -> their 30 KCS features  */
                                  /* (special_KCS_Input_transform, R/models_Fk_GAN/Fk_discriminator.py:36-146) in buffer   */
                                  /* dst, columns 30..63 zero: the 3D critic's KCS branch without a launch of its own        */
#define DHAUG_MLP_F_OUT_F32   4   /* network output (n <= 64): fp32 (M, ld) to g, staged through buffer dst (0 or 1)    */
#define DHAUG_MLP_F_DOT_OUT  16   /* GEMM whose only consumer is a 1-wide linear layer (a critic's logit): the activation  */
                                  /* is not stored; its dot product with w2 = fp32 [257] (that layer's weights as bf16      */
                                  /* values, zero beyond n, bias at [256]) goes to g (M, ld) column 0 as fp32; dst (0 or 1,  */
                                  /* not src / res) is scratch for the partial sums                                          */
typedef struct dhaug_mlp_unit {
    int kind, flags;
    int src, dst, res;            /* buffer ids, -1 = none; dst may equal res (in-place residual), never src        */
    int src2, ksteps2;            /* optional second source (input = concatenation of two buffers); ksteps2 = 0: none */
    int ksteps;                   /* K/16 of the first source (K zero-padded to 16 by the producer)                  */
    int n;                        /* output features of the layer (<= 256)                                          */
    int act;                      /* DHAUG_ACT_*                                                                     */
    float slope;
    int cols;                     /* LOAD/STORE: columns moved (multiple of 8)                                       */
    int64_t ld;
    const void* g;                /* global tensor of LOAD / STORE / OUT_F32                                         */
    const void* w;                /* GEMM: packed fragments of the first source's weight columns (dhaug_pack_wfrag)  */
    const void* w2;               /* fragments of the second source's weight columns                                 */
    const float* bias;            /* GEMM: fp32 [256], zero padded                                                   */
    void* save;                   /* GEMM (dhaug_mlp_forward, not OUT_F32 / DOT_OUT), optional: the layer's output also   */
    int64_t save_ld;              /* goes to global memory as bf16 (M, save_ld), columns [0, ceil16(n)) (zero beyond n):   */
                                  /* forward-with-save of the training step (the saved activations of                     */
                                  /* R/models_Fk_GAN/model_fk_gan_train.py:177-230's autograd graph)                      */
    void* bits;                   /* GEMM with `save`, a full-width (n > 224) layer INSIDE a run of such layers, optional:   */
                                  /* one bit per output element, (y > 0) -- the mask act'(y) of the backward and tangent       */
                                  /* sweeps in 1/16 of the bytes.  uint32 [ceil(M/128)*4][4][64]: word ((T*4 + w)*64 + l) of  */
                                  /* 32-row tile T covers row 32 T + (l & 31), features 32 (w + 4 t) + 8 g + 4 (l >> 5) + e;   */
                                  /* element j = 16 t + 4 g + e sits at bit j/2 (j even) or 16 + j/2 (j odd).  Consumed by    */
                                  /* dhaug_gemm_bf16_dbits.  A unit that is not such a layer -> DHAUG_EUNSUPPORTED.          */
    int64_t save_rows;            /* with `save`: 0 = every row is saved; n > 0 = rows [0, n) only; < 0 = none (the sign bits are   */
                                  /* written for every row regardless).  The interpolated rows of a critic step's batch are read   */
                                  /* back by nothing but their masks: R/models_Fk_GAN/Fk_discriminator.py:205-231 needs D(x_hat)'s  */
                                  /* input gradient, not its activations.                                                          */
} dhaug_mlp_unit;

/* dhaug_pack_wfrag for every layer of a network in one launch (after each optimizer step of a training loop that runs the
 * fused programs: R/models_Fk_GAN/model_fk_gan_train.py:177-230 steps the critics every iteration).  Per descriptor: the
 * fragment blob of W[:, k0:k0+K] (ksteps = K padded to multiples of 64, in units of 16; always 8 slices), the zero-padded
 * fp32 bias [256] (bias_dst, optional) and, for a 1-wide logit layer folded into its producer, the DOT_OUT vector [257]
 * (dot_dst, optional).  descs_device: array of n descriptors in device memory.
 * Second operand (W2 != NULL): the descriptor stands for the composite of two linear layers with nothing between them,
 * y = W (W2 x + bias2) + bias: W is [N, ldw >= K2], W2 is [K2, ldw2], and (k0, K) selects columns of W2.  The blob holds
 * bf16( (W W2)[n][k0 + k] ) and bias_dst W bias2 + bias; see dhaug_pack_wfrag_composed for the precision.  W2 == NULL: one
 * layer, the other three fields are not read. */
typedef struct dhaug_wfrag_desc {
    const float* W;
    int64_t ldw;
    void* dst;
    const float* bias;
    float* bias_dst;
    float* dot_dst;
    int32_t N, K, k0, ksteps;
    const float* W2;              /* composite: the layer applied FIRST, [K2, ldw2]; NULL: a single layer              */
    const float* bias2;           /* its bias [K2] (optional)                                                          */
    int64_t ldw2;
    int32_t K2;                   /* inner width: output features of W2 = input features of W                          */
    int32_t pad_;
} dhaug_wfrag_desc;
int dhaug_pack_wfrag_batch(const dhaug_wfrag_desc* descs_device, int n, void* stream);

/* Fragment blob (layout of dhaug_pack_wfrag) and zero-padded fp32 bias [256] of the composite of two nn.Linear layers with no
 * activation, residual or consumer between them: y = Wa (Wb x + bias_b) + bias_a, Wa [N, ldwa >= Ki], Wb [Ki, ldwb >= k0 + K].
 *   dst      <- bf16( sum_m Wa[n][m] Wb[m][k0 + k] ),   bias_dst[n] <- sum_m Wa[n][m] bias_b[m] + bias_a[n]   (biases optional)
 * Precision: formed from the fp32 parameters, every sum accumulated in fp64 in the order m = 0 .. Ki-1, rounded to fp32 and then
 * ONCE to bf16 -- neither factor is rounded to bf16 on its own, and the intermediate activation Wb x + bias_b, which a chain of
 * two layers rounds to bf16, does not exist.  The same device routine serves a descriptor with W2 set in dhaug_pack_wfrag_batch:
 * identical bits.  N <= 256, K <= 256. */
int dhaug_pack_wfrag_composed(const float* Wa, int64_t ldwa, const float* bias_a, const float* Wb, int64_t ldwb, const float* bias_b,
                              uint16_t* dst, float* bias_dst, int64_t N, int64_t Ki, int64_t K, int64_t k0, void* stream);

/* Runs the program on every 128-row tile of the batch: replaces the nn.Sequential / myResNet stacks of
 * R/models_Fk_GAN/Fk_generator.py:115-119, Fk_discriminator.py:180-201 and :253-266 (inference / sampling passes).
 * bf16 operands, fp32 accumulate, bf16 activations between layers -- the same arithmetic as a chain of
 * dhaug_gemm_bf16 calls over the layers the program holds (a caller may hand over two layers with nothing between them as one:
 * dhaug_pack_wfrag_composed). */
int dhaug_mlp_forward(const dhaug_mlp_unit* units, int nunits, int64_t M, void* stream);

/* Host only, launches nothing: the validation of dhaug_mlp_forward and its planning pass over the same program; plans_out[i]
 * receives how unit i would be executed (an internal encoding, stable enough for tests: bit 13 = a run of full-width layers,
 * DHAUG_MLP_PLAN_LEADG on a bf16 LOAD = the LOAD and the stack behind it run as one unit whose lead layer reads the tensor
 * from global memory instead of an LDS image; DHAUG_MLP_PLAN_VSTORE on an fp32 output layer (DHAUG_MLP_F_OUT_F32, also where it
 * runs as a stack's tail) = an inference launch whose output rows are contiguous (ld == n, 16-byte aligned g): the tile leaves
 * as 16-byte groups, not dword by dword; DHAUG_MLP_NOVSTORE in the environment clears it).  No pointer of the program is dereferenced.  Returns what dhaug_mlp_forward
 * would return in front of its launch. */
#define DHAUG_MLP_PLAN_STACK  (1 << 13)
#define DHAUG_MLP_PLAN_LEADG  (1 << 15)
#define DHAUG_MLP_PLAN_VSTORE (1 << 8)
int dhaug_mlp_plan(const dhaug_mlp_unit* units, int nunits, int64_t M, int32_t* plans_out);

/* Parity-grade variant of the same programs: every operand is an fp16 pair x = hi + lo (22 mantissa bits), a product is
 * Whi Xhi + Whi Xlo + Wlo Xhi on v_mfma_f32_32x32x16_f16 with fp32 accumulation -- fp32-grade results (the reference's
 * layers are fp32 nn.Linear: R/models_Fk_GAN/Fk_discriminator.py:180-201,253-266, R/models_Fk_GAN/Fk_generator.py:115-119;
 * tolerance 1e-4 relative on the logits) at three matrix instructions per k-step.  128-row batch tiles; the activation lives
 * in ONE hi / lo image in LDS that every layer updates in place, so the three buffer ids of a program are virtual: the
 * library checks that every value a unit reads is where the kernel can find it (the image for a source; for a residual the
 * registers of the lane that produced it, or the workspace) and returns DHAUG_EUNSUPPORTED otherwise.  A value that a later
 * unit adds as a RESIDUAL stays in registers.  Only a partial sum that is PARKED while another branch of the program uses the
 * image and those registers (a result that is added later and read as a source by nobody) waits in a global workspace (fp32,
 * written and read back by the same lane; only the second half of the buffer is touched).  Both are read back lane by lane,
 * so the unit that adds a value must deal its blocks to the waves as the unit that wrote it did: n of both in the same one of
 * 1..32, 33..64, 65..128, 129..256 (DHAUG_EUNSUPPORTED otherwise).  A unit that adds a residual or a parked sum always leaves
 * its own result in those registers: a kept value that a later unit would add once more is DHAUG_EUNSUPPORTED.
 * A program with residuals or a
 * parked sum passes g = a 16-byte aligned buffer of DHAUG_MLP_X3_WORKSPACE_BYTES, shared with no concurrent launch, in its
 * GEMM units that are not outputs (any content).
 * Differences from dhaug_mlp_forward: weights come from dhaug_pack_wfrag_f16x2; only LOAD_F32 (cols and ld even, 8-byte
 * aligned base), LOAD_KCS and GEMM units; no second source; no F_DOT_OUT (a 1-wide logit layer is an OUT_F32 unit).
 * dhaug_pack_wfrag_f16x2: dst[(((slice*ksteps + ks)*2 + piece)*64 + lane)*8 + j] = piece(W[32 slice + (lane&31)][k0 + 16 ks +
 * 8 (lane>>5) + j]), piece 0 = fp16(w), piece 1 = fp16(w - piece 0); 8 slices, k-steps padded to multiples of 4, i.e.
 * 2 * 8 * ksteps * 512 fp16 values. */
int dhaug_pack_wfrag_f16x2(const float* W, int64_t ldw, uint16_t* dst, int64_t N, int64_t K, int64_t k0, void* stream);
/* The same pair of pieces in the fragment order of v_mfma_f32_16x16x32_f16 (same size): per slice of 32 features two feature
 * tiles of 16, k-steps of 32 -- dst[((((slice*2 + ft)*(ksteps/2) + ks)*2 + piece)*64 + lane)*8 + j] = piece(W[32 slice + 16 ft +
 * (lane&15)][k0 + 32 ks + 8 (lane>>4) + j]).  A program whose GEMM units carry DHAUG_MLP_F_T16 (all of them or none) runs its
 * layers on that instruction: same image, same results to rounding (k is summed 32 at a time), and -- measured, MI355X,
 * tools/ubench/mfma_shape.hip -- 1.19 x the FLOP/s of the 32 x 32 x 16 form at equal cycles, because the chip holds a higher
 * clock on it. */
#define DHAUG_MLP_F_T16      32
int dhaug_pack_wfrag_f16x2_t16(const float* W, int64_t ldw, uint16_t* dst, int64_t N, int64_t K, int64_t k0, void* stream);
#define DHAUG_MLP_X3_WORKSPACE_BYTES (2 * 256 * 4 * 64 * 128 * 4)   /* regions x workgroups x waves x lanes x values x 4 */
int dhaug_mlp_forward_x3(const dhaug_mlp_unit* units, int nunits, int64_t M, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Elementwise / reductions used by the training step
 * ---------------------------------------------------------------------------------------------------- */

/* column sums: src (M, N) fp32|bf16 -> dst[N] fp32 (bias gradients). */
int dhaug_colsum_f32(const float* src, int64_t ld, float* dst, int64_t M, int64_t N, int accumulate,
                     void* stream);
int dhaug_colsum_bf16(const uint16_t* src, int64_t ld, float* dst, int64_t M, int64_t N, int accumulate,
                      void* stream);

/* dst = g * act'(y)  (y = the saved activation output; relu: y>0, lrelu: y>0 ? 1 : slope), bf16 in/out,
 * optional second output g_res (same values) is the gradient flowing into a residual branch. */
int dhaug_act_backward_bf16(const uint16_t* g, int64_t ld_g, const uint16_t* y, int64_t ld_y,
                            uint16_t* dst, int64_t ld_dst, int64_t M, int64_t N, int act, float slope,
                            void* stream);

/* fp32 variant on flat arrays of n elements. */
int dhaug_act_backward_f32(const float* g, const float* y, float* dst, int64_t n, int act, float slope,
                           void* stream);

/* Fused Adam step on a flat fp32 parameter vector (torch.optim.Adam semantics, eps outside the sqrt,
 * bias correction; R/models_Fk_GAN/model_fk_gan_train.py:112-118: lr 1e-4, betas (0.5, 0.9)).
 * grad_scale multiplies the gradient first (1/world_size after an all-reduce sum). */
int dhaug_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                    float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* stream);

/* The same step with the step count in device memory (*step_dev >= 1, advanced with dhaug_counter_add before the call): a
 * captured hipGraph replays the launch, so the bias corrections must not be baked into kernel arguments. */
int dhaug_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                        float lr, float beta1, float beta2, float eps, const int* step_dev, float grad_scale, void* stream);
int dhaug_counter_add(int* counter, int value, void* stream);

/* The bf16 operand copies of ALL weights of a network in two launches (after its Adam step): per weight W (N, K) fp32,
 * contiguous: nt = bf16 (N, Kp) zero-padded along K (operand of x W^T), nn = bf16 (K, Np) = W^T zero-padded along N (operand
 * of g W); Kp, Np multiples of 16.  descs_device: array of nparams descriptors in device memory. */
typedef struct dhaug_repack_desc {
    const float* W;
    void* nt;
    void* nn;
    int N, K, Kp, Np;
} dhaug_repack_desc;
int dhaug_repack_weights(const dhaug_repack_desc* descs_device, int nparams, void* stream);

/* The optimizer step of a whole network as two streaming launches (replaces dhaug_counter_add + dhaug_adam_step_dev +
 * dhaug_repack_weights; same arithmetic, torch.optim.Adam.step at R/models_Fk_GAN/model_fk_gan_train.py:218,470): Adam on the flat
 * vectors with the bf16 copy nt of every weight written from the updated values, then nn = nt^T.
 * descs_device (device memory, ndesc entries, ascending item0, together covering every element of the flat vectors exactly once):
 * a weight W (N, K) at element offset `off` with its copy nt (N, Kp) as in dhaug_repack_desc, items = ceil(N * Kp / 4096); or
 * N = 0: `len` plain elements at `off`, items = ceil(len / 4096).  nitems = the sum.  weights_device: the dhaug_repack_desc of the
 * same weights (nweights of them), for the transposed copies.  state: the step count in device memory; the call uses count + 1
 * for the bias corrections and leaves count + 1 there -- a captured hipGraph replays it. */
typedef struct dhaug_adam_desc {
    long long off, len;
    void* nt;
    int N, K, Kp, pad_;
    long long item0;
} dhaug_adam_desc;
int dhaug_adam_repack_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                           float eps, int* state, float grad_scale, const dhaug_adam_desc* descs_device, int ndesc, int64_t nitems,
                           const dhaug_repack_desc* weights_device, int nweights, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * WGAN-GP critic step arithmetic (R/models_Fk_GAN/Fk_discriminator.py:205-231, model_fk_gan_train.py:186-221)
 * ---------------------------------------------------------------------------------------------------- */

/* out (3B, W) fp32: rows [0,B) = real, [B,2B) = fake, [2B,3B) = alpha_b * real + (1 - alpha_b) * fake -- the batch one
 * critic step scores (the two critic passes and the penalty's interpolates as one batch). */
int dhaug_gp_assemble(const float* real, const float* fake, const float* alpha, float* out, int64_t B, int64_t W, void* stream);
/* ... and rows [0, 2B) (real, fake) once more as bf16 (2B, ld_bf16 >= W; columns beyond W are not written): the operand the step's
 * weight-gradient sweep contracts the input layer's cotangent with, without a cast launch of its own (same rounding: nearest even) */
int dhaug_gp_assemble_bf16(const float* real, const float* fake, const float* alpha, float* out, uint16_t* rows_bf16, int64_t ld_bf16,
                           int64_t B, int64_t W, void* stream);

/* Per row b of grad (B, W) = dD/dx_hat:  n = ||grad_b||_2;  pen[b] = (n - 1)^2;  v_b = coef * (n - 1) / n * grad_b, the
 * cotangent of the penalty on grad (coef = 2 * LAMBDA / B gives d/dgrad of LAMBDA * mean((n - 1)^2)). */
int dhaug_gp_penalty(const float* grad, float* v, float* pen, int64_t B, int64_t W, float coef, void* stream);
/* ... with v also as bf16 (B, ld_bf16 >= W): the tangent sweep's first operand */
int dhaug_gp_penalty_bf16(const float* grad, float* v, uint16_t* v_bf16, int64_t ld_bf16, float* pen, int64_t B, int64_t W, float coef,
                          void* stream);

/* Frame differences of clips (the motion critics' diff branches, R/models_Fk_GAN/Fk_discriminator.py:458-460,489-492,570-573):
 * x (rows, R*in_w) -> out (rows, (R-1)*w), out[r][f][c] = x[r][f+1][c] - x[r][f][c] over the first w columns of every frame;
 * adjoint != 0: the transposed map, x (rows, (R-1)*w) -> out (rows, R*in_w) (zero for columns >= w). */
int dhaug_frame_diff(const float* x, float* out, int64_t rows, int R, int in_w, int w, int adjoint, void* stream);

/* Frame reversal of clips, x (rows, R*w) -> out[r][f][:] = x[r][R-1-f][:] (torch.flip(dims=[1]) of the video loop's playback
 * copies, R/models_Fk_GAN/video_GAN_fun.py:467,521); the map is its own transpose, so the same call back-propagates. */
int dhaug_frame_reverse(const float* x, float* out, int64_t rows, int R, int w, void* stream);

/* out[0] = sum_i weights[i] * mean(arrays[i][0 .. counts[i])): the generator loss gen_loss (or -gen_loss) from the critics'
 * logit arrays in one launch (R/models_Fk_GAN/model_fk_gan_train.py:470-476).  arrays / counts / weights: HOST arrays of
 * n <= DHAUG_WEIGHTED_MEANS_MAX entries (read during the call); the logit arrays and out are device memory. */
#define DHAUG_WEIGHTED_MEANS_MAX 16
int dhaug_weighted_means(const float* const* arrays, const int64_t* counts, const float* weights, int n, float* out, void* stream);

/* out5 = { D_real, D_fake, GP = lambda * mean(pen), Wasserstein_D = D_real - D_fake, D_cost = D_fake - D_real + GP } from
 * the logits (rows [0,B) real, [B,2B) fake, stride ld) and the P per-row penalties (P = B, or B * frames for the 2D motion
 * critic, whose penalty is taken per frame). */
int dhaug_critic_scalars(const float* logits, int64_t ld, const float* pen, int64_t B, int64_t P, float lambda, float* out5,
                         float* scratch /* DHAUG_CRITIC_SCALARS_SCRATCH floats, any content */, void* stream);
#define DHAUG_CRITIC_SCALARS_SCRATCH 192

/* The TOP of a branch critic -- merge layer (concatenation of two 256-wide branches -> n0 <= 112 features), one n0-wide myResNet
 * block, the 1-wide logit layer (R/models_Fk_GAN/Fk_discriminator.py:149-201: merge_previous, merge_block1, output) -- in the
 * explicit training step, ONE launch per sweep; the n0-wide tensors stay in LDS between the layers, results bit-identical to the
 * launches replaced (dhaug_rank1_mask_bf16 + three dhaug_gemm_bf16_dmask_pad / dhaug_gemm_bf16_dbits_wide calls).
 *   dhaug_critic_top_backward_bf16 (sweep 2):
 *     g2 = bf16(seed w_out) * act'(m1);  g1 = (g2 W2^T) * act'(mh);  g0 = (g1 W1^T + g2) * act'(m0);  gcat = (g0 Wm^T) * act'(cat)
 *     with W2 / W1 (n0, >= 112) and Wm (512, >= 112) the operand copies whose ROWS are the product's outputs (the "nn" copies of
 *     merge_block1.fc2 / fc1 and merge_previous), the masks of the concatenation as the two sign-bit arrays of its 256-column blocks
 *     (struct dhaug_mlp_unit.bits).  m1, mh, m0: the saved activations (M, ld_m) bf16; g2, g1, g0 (M, ld_g) bf16 with zero columns
 *     [n0, 112); gcat (M, ld_gcat >= 512).  M a multiple of 64 (DHAUG_EUNSUPPORTED otherwise: the caller uses the separate launches).
 * All matrices bf16 with 16-byte aligned rows. */
typedef struct dhaug_top_desc {
    const uint16_t* seed; int64_t ld_seed;              /* (M, >= 1): column 0 = the logit cotangent of the row */
    const uint16_t* wout; int64_t ld_wout;              /* the logit layer's n0 weights, element stride ld_wout */
    const uint16_t* x; int64_t ldx;                     /* tangent sweep: the tangent of the concatenation (M, 512) */
    const uint16_t* m1; const uint16_t* mh; const uint16_t* m0; int64_t ld_m;
    const uint16_t* w2; int64_t ldw2;
    const uint16_t* w1; int64_t ldw1;
    const uint16_t* wm; int64_t ldwm;
    const uint32_t* bits0; const uint32_t* bits1;
    uint16_t* g2; uint16_t* g1; uint16_t* g0; int64_t ld_g;
    uint16_t* gcat; int64_t ld_gcat;
    int64_t M; int64_t n0; int64_t nc;                  /* nc = 512 */
    int32_t mask_act; float mask_slope;
} dhaug_top_desc;
int dhaug_critic_top_backward_bf16(const dhaug_top_desc* d, void* stream);
/*   dhaug_critic_top_tangent_bf16 (sweep 3, rows = the interpolated rows): IN PLACE over the rows of the saved activations,
 *     m0 <- (x Wm^T) * act'(m0);  mh <- (m0' W1^T) * act'(mh);  m1 <- (mh' W2^T + m0') * act'(m1)      (primes: the values just written)
 *     x (M, ldx >= 512) the tangent of the concatenation; Wm (n0, >= 512), W1 / W2 (n0, >= 112) the "nt" operand copies (rows = the
 *     layer's outputs).  Replaces one dhaug_gemm_bf16_dmask_pad with K = 512 and two with K = 112 (the second with the skip); same bits. */
int dhaug_critic_top_tangent_bf16(const dhaug_top_desc* d, void* stream);

/* The 3D critic's gradient penalty between its backward chain and its tangent sweep in ONE launch (R/models_Fk_GAN/Fk_discriminator.py:
 * 205-231 with the KCS transform of :81-140): g = KCS^T(pose) grad_kcs + grad_pose = dD/dx_hat (N, 48); pen[b] = (||g_b|| - 1)^2;
 * v_b = coef (||g_b|| - 1) / ||g_b|| g_b (0 where the norm is 0); tan_kcs = dKCS(pose)[v].  grad_kcs (N, 30): cosines then lengths;
 * outputs: tan_kcs_bf16 (N, 32) and tan_pose_bf16 = v (N, 48) as the bf16 operands of the tangent sweep's first layers, pen (N) fp32.
 * The operations of dhaug_kcs_backward + dhaug_add_f32 + dhaug_gp_penalty + dhaug_kcs_jvp + two dhaug_cast_pad_bf16 calls in their order (fp32
 * results equal to the last bit or two: the compiler contracts multiply-adds per kernel). */
int dhaug_d3_penalty(const float* pose16, const float* grad_kcs, const float* grad_pose, float coef, uint16_t* tan_kcs_bf16,
                     uint16_t* tan_pose_bf16, float* pen, int64_t N, void* stream);

/* First step of a critic's backward chain, through its 1-wide logit layer: out[r][c] = bf16(seed[r] * w[c]) * act'(mask[r][c])
 * for c < N, zero in [N, pad_cols) -- (gz W_out) * act'(y) of R/models_Fk_GAN/Fk_discriminator.py:201,266's backward, which as
 * a GEMM has K = 1.  seed: bf16, one value per row (stride ld_seed); w: the layer's N weights as bf16 (stride ld_w); mask, out:
 * bf16 (M, ld) with 16-byte aligned rows; pad_cols <= 1024 (DHAUG_EUNSUPPORTED beyond). */
int dhaug_rank1_mask_bf16(const uint16_t* seed, int64_t ld_seed, const uint16_t* w, int64_t ld_w, const uint16_t* mask, int64_t ld_mask,
                          uint16_t* out, int64_t ld_out, int64_t M, int64_t N, int64_t pad_cols, int mask_act, float mask_slope,
                          void* stream);
/* The same for a 256-wide hidden layer whose mask is a sign-bit array (struct dhaug_mlp_unit.bits): no mask image is read. */
int dhaug_rank1_bits_bf16(const uint16_t* seed, int64_t ld_seed, const uint16_t* w, int64_t ld_w, const uint32_t* bits,
                          uint16_t* out, int64_t ld_out, int64_t M, int mask_act, float mask_slope, void* stream);

/* out = a + b over n fp32 values (the branch contributions to dD/dx_hat of a multi-branch critic). */
int dhaug_add_f32(const float* a, const float* b, float* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Single-frame VideoPose posenet: BatchNorm1d (batch statistics) + ReLU + Dropout (+ residual) between two GEMMs
 * (R/models_baseline/videopose/model_VideoPose3D.py:163-220, TemporalModelOptimized1f._forward_blocks; every convolution there has
 * kernel width 1 on a length-1 sequence, i.e. is a dense layer: dhaug_gemm_bf16)
 * ----------------------------------------------------------------------------------------------------
 * z, g, residual: (M, C) row-major with a leading dimension (elements), fp32 (z_bf16 = 0) or bf16 (z_bf16 = 1) -- all three of the
 * one type; rows start 16-byte aligned (base 16-byte aligned, ld * element size % 16 == 0) and ld >= C (DHAUG_EALIGN otherwise).
 * No column at or beyond C of any input row is read.  Outputs: bf16 (M, ld >= ceil16(C), ld % 8 == 0), columns [C, ceil16 C) written
 * as zeros (directly the next GEMM's operand), and / or fp32 (M, ld >= C, ld % 4 == 0); at least one of the two.
 * workspace: device, DHAUG_BN_MAX_CHUNKS * 2 * C doubles, 8-byte aligned: the per-chunk column sums between the two launches of a
 * pass (stream order; one pass at a time per workspace).  fp64 accumulation in a fixed order, no atomics: the same call gives the
 * same bits.  IEEE arithmetic; the kernels' own NaN convention: a NaN pre-activation is a NaN in y, and fails the backward pass's
 * (pre > 0) test, so gz is 0 there.
 *
 * dhaug_bn_partials + dhaug_bn_act_forward (same z, M, C, workspace): mean = sum z / M, var = sum z^2 / M - mean^2 (biased),
 *   rstd = 1 / sqrt(var + eps), each rounded to fp32 once from fp64;
 *     y = keep * relu(fma(fl((z - mean) * rstd), gamma, beta)) * fl(1 / (1 - p)) (+ residual).
 *   mean, rstd (C fp32 each) are written for the backward pass; running_mean / running_var (optional, both or neither) are updated as
 *   nn.BatchNorm1d does, r = (1 - momentum) * r + momentum * (mean | var * M / (M - 1)), and *num_batches_tracked (optional, device
 *   int64) is advanced by one.  M = 1 with batch statistics: DHAUG_EUNSUPPORTED (nn.BatchNorm1d raises).
 *   workspace = NULL is the given-statistics mode: mean and rstd are READ, no buffer may be passed, one launch.
 *   Dropout: keep iff word >= (uint32)(p * 2^32) with Philox4x32-10, key = seed, counter = (element index / 4, offset), element
 *   index = row * C + column, the four words of a call deciding four consecutive elements; 0 <= p < 1 (DHAUG_EINVAL otherwise);
 *   p = 0 draws nothing and multiplies by nothing.
 * dhaug_bn_act_backward_partials + dhaug_bn_act_backward (same arguments): g is the cotangent of the branch output (the
 *   residual's cotangent is g itself).  The pre-activation is recomputed by the forward kernel's own expression and the keep
 *   decision from (seed, offset): gz = g * keep / (1 - p) where the pre-activation is > 0, exactly 0 elsewhere; xhat = (z - mean) * rstd;
 *     dz = (gamma * rstd) * ((gz - sum gz / M) - xhat * sum(gz xhat) / M),  dgamma = sum gz xhat,  dbeta = sum gz  (optional).
 * dhaug_bn_fold (evaluation): W_out[n, :] = gamma[n] * rstd_run[n] * W[n, :] (N, K) fp32, bias_out[n] = beta[n] - running_mean[n] *
 *   gamma[n] * rstd_run[n], rstd_out[n] = rstd_run[n] = 1 / sqrt(running_var[n] + eps); each output optional (at least one), each
 *   value formed in fp64 and rounded once.
 * dhaug_bn_fold_bias: dhaug_bn_fold for a layer that has a bias of its own in front of the BatchNorm (the nn.Linear layers of
 *   R/models_baseline/mlp/linear_model.py), layer_bias (N fp32, optional) behind W, ldw.  W_out and rstd_out as dhaug_bn_fold;
 *     bias_out[n] = beta[n] + (layer_bias[n] - running_mean[n]) * gamma[n] * rstd_run[n],
 *   formed in fp64 and rounded once.  layer_bias = NULL is a zero bias: dhaug_bn_fold's own launch, every output bit-identical to
 *   its.  The same codes and alignment rules (layer_bias 4-byte aligned); N = 0 is a no-op that looks at no pointer.
 * All: DHAUG_EINVAL for M, C, N, K < 0, a z_bf16 outside {0, 1}, p outside [0, 1), a NULL required pointer, no output; an empty
 * batch (M = 0 or C = 0; N = 0) is a no-op that looks at no pointer. */
#define DHAUG_BN_MAX_CHUNKS 32
int dhaug_bn_partials(const void* z, int z_bf16, int64_t ld_z, int64_t M, int64_t C, void* workspace, void* stream);
int dhaug_bn_act_forward(const void* z, int z_bf16, int64_t ld_z, const void* residual, int64_t ld_res, const float* gamma,
                         const float* beta, float* mean, float* rstd, const void* workspace, float* running_mean,
                         float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float p, uint64_t seed,
                         uint64_t offset, uint16_t* y_bf16, int64_t ld_yb, float* y_f32, int64_t ld_yf, int64_t M, int64_t C,
                         void* stream);
int dhaug_bn_act_backward_partials(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g, const float* gamma,
                                   const float* beta, const float* mean, const float* rstd, float p, uint64_t seed,
                                   uint64_t offset, int64_t M, int64_t C, void* workspace, void* stream);
int dhaug_bn_act_backward(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g, const float* gamma,
                          const float* beta, const float* mean, const float* rstd, float p, uint64_t seed, uint64_t offset,
                          const void* workspace, uint16_t* dz_bf16, int64_t ld_dzb, float* dz_f32, int64_t ld_dzf, float* dgamma,
                          float* dbeta, int64_t M, int64_t C, void* stream);
/* The device-stream forms of the three launches above (dhaug_bn_act_forward, dhaug_bn_act_backward_partials, dhaug_bn_act_backward):
 * the same kernels instantiated a second time, with (seed, offset) replaced by (rng_cell, delta).  rng_cell: two device uint64
 * {seed, base}, 8-byte aligned (DHAUG_EALIGN otherwise); the launch uses seed = rng_cell[0] and offset = rng_cell[1] + delta, a full
 * 64-bit sum, read when it runs -- so a captured launch draws a new mask at every replay once the base has been advanced
 * (dhaug_u64_add).  For equal (seed, offset) every output is bit-identical to the entry it mirrors.  p = 0: the cell is not read and
 * may be NULL; p > 0 with a NULL cell: DHAUG_EINVAL before any launch.  Every other argument, check and code is the mirrored entry's. */
int dhaug_bn_act_forward_dr(const void* z, int z_bf16, int64_t ld_z, const void* residual, int64_t ld_res, const float* gamma,
                            const float* beta, float* mean, float* rstd, const void* workspace, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float p,
                            const uint64_t* rng_cell, uint64_t delta, uint16_t* y_bf16, int64_t ld_yb, float* y_f32, int64_t ld_yf,
                            int64_t M, int64_t C, void* stream);
int dhaug_bn_act_backward_partials_dr(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g, const float* gamma,
                                      const float* beta, const float* mean, const float* rstd, float p, const uint64_t* rng_cell,
                                      uint64_t delta, int64_t M, int64_t C, void* workspace, void* stream);
int dhaug_bn_act_backward_dr(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g, const float* gamma,
                             const float* beta, const float* mean, const float* rstd, float p, const uint64_t* rng_cell,
                             uint64_t delta, const void* workspace, uint16_t* dz_bf16, int64_t ld_dzb, float* dz_f32, int64_t ld_dzf,
                             float* dgamma, float* dbeta, int64_t M, int64_t C, void* stream);
int dhaug_bn_fold(const float* W, int64_t ldw, const float* gamma, const float* beta, const float* running_mean,
                  const float* running_var, float eps, float* W_out, int64_t ld_out, float* bias_out, float* rstd_out, int64_t N,
                  int64_t K, void* stream);
int dhaug_bn_fold_bias(const float* W, int64_t ldw, const float* layer_bias, const float* gamma, const float* beta,
                       const float* running_mean, const float* running_var, float eps, float* W_out, int64_t ld_out,
                       float* bias_out, float* rstd_out, int64_t N, int64_t K, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Multi-frame VideoPose posenets: the tap layout around the GEMMs (R/models_Fk_GAN/mulit_farme_videopose.py; csrc/dhaug_taps.hip)
 * ----------------------------------------------------------------------------------------------------
 * With activations as rows (batch-major, then time) a k-tap Conv1d is  A W2d^T,  W2d[n, j Cin + c] = W[n, c, j], where row r of A is
 * the concatenation of the k input rows of output r's window.  With stride = k over non-overlapping frames (the training model) A is
 * the input itself, viewed (M / k, k Cin); otherwise (dilation, the evaluation model) dhaug_tap_gather builds it.  Data movement only,
 * vector stores, no atomics.
 *
 * dhaug_conv_taps_pack_bf16: W fp32 (N, Cin, k) contiguous ->
 *     nt (N, ld_nt >= k Cin) bf16, nt[n, j Cin + c] = bf16(W[n, c, j])                          (the B operand of x W2d^T);
 *     nn (k Cin, ld_nn >= ceil16 N) bf16, optional, nn[j Cin + c, n] = the same value, columns [N, ceil16 N) zero
 *                                                                                                 (the B operand of g W2d).
 *   Columns of nt at and beyond k Cin and of nn at and beyond ceil16 N are not touched.  Rounding as dhaug_cast_pad_bf16: the two
 *   outputs equal dhaug_cast_pad_bf16 / dhaug_cast_transpose_bf16 of the permuted matrix bit for bit.  W is read once.
 *   DHAUG_EINVAL: N or Cin < 0, a NULL W or nt, a leading dimension below its minimum.  DHAUG_EUNSUPPORTED: k outside [1, 16],
 *   Cin % 16 != 0, N Cin k >= 2^31.  DHAUG_EALIGN: W, nt or nn not 16-byte aligned, ld_nt or ld_nn no multiple of 8.
 * dhaug_conv_taps_permute_f32: fp32, both matrices contiguous, any N, Cin, k >= 1.
 *     to_taps = 1:  dst (N, k Cin),  dst[n, j Cin + c]  = src[n, c, j]        (src (N, Cin, k); accumulate must be 0);
 *     to_taps = 0:  dst (N, Cin, k), dst[n, c, j] (+)= src[n, j Cin + c]      (src (N, k Cin); accumulate 1 adds into dst, each thread
 *                                                                              reading and writing only its own elements).
 *   DHAUG_EINVAL: a negative size, a flag outside {0, 1}, accumulate with to_taps, a NULL pointer, src == dst.  DHAUG_EUNSUPPORTED:
 *   N Cin k >= 2^31.  DHAUG_EALIGN: src not 4-byte, dst not 16-byte aligned.
 * dhaug_tap_gather: x (nseq t_in, ld_x >= C) fp32 (x_bf16 = 0) or bf16 (1), nseq sequences of t_in rows each ->
 *     out[(s t_out + t), j C + c] = x[(s t_in + t stride + j dilation), c],   t_out = (t_in - (k - 1) dilation - 1) / stride + 1,
 *   to out_bf16 (nseq t_out, ld_ob >= k C) and / or out_f32 (nseq t_out, ld_of >= k C); at least one.  bf16 from bf16 is a copy, bf16
 *   from fp32 rounds as dhaug_cast_pad_bf16, out_f32 needs fp32 input (DHAUG_EINVAL otherwise).  No window reads across a sequence
 *   boundary: the last row read of sequence s is s t_in + t_in - 1 at most.  Columns at and beyond k C of the outputs are not touched.
 *   DHAUG_EINVAL: a negative size, dilation or stride < 1, x_bf16 outside {0, 1}, a NULL x, no output, a leading dimension below
 *   its minimum.  DHAUG_EUNSUPPORTED: C % 16 != 0, k outside [1, 16], t_in < (k - 1) dilation + 1 (t_out < 1), nseq t_in >= 2^31,
 *   k C >= 2^28, dilation or stride >= 2^30.  DHAUG_EALIGN: a pointer not 16-byte aligned, rows not 16-byte aligned (ld_x, ld_ob % 8
 *   for bf16, ld_x, ld_of % 4 for fp32).
 * All three: an empty problem (N or Cin = 0, for the permutation also k = 0; nseq or C = 0) is a no-op that looks at no pointer. */
int dhaug_conv_taps_pack_bf16(const float* W, int64_t N, int64_t Cin, int k, uint16_t* nt, int64_t ld_nt, uint16_t* nn,
                              int64_t ld_nn, void* stream);
int dhaug_conv_taps_permute_f32(const float* src, float* dst, int64_t N, int64_t Cin, int k, int to_taps, int accumulate,
                                void* stream);
int dhaug_tap_gather(const void* x, int x_bf16, int64_t ld_x, int64_t nseq, int64_t t_in, int64_t C, int k, int dilation,
                     int stride, uint16_t* out_bf16, int64_t ld_ob, float* out_f32, int64_t ld_of, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * SemGCN posenet: the joint mix of a semantic graph convolution (R/models_baseline/gcn/sem_graph_conv.py; csrc/dhaug_graph.hip)
 * ----------------------------------------------------------------------------------------------------
 * Activations are rows, pose-major then joint: row 16 b + i is joint i of pose b, M = 16 x poses (DHAUG_EINVAL otherwise).  A is the
 * layer's 16 x 16 adjacency, fp32, row-major, on the device.  With H = x Wcat^T = [h0 | h1] (M, 2C) from the GEMM in front,
 *     z[b,i,:] = A[i,i] h0[b,i,:] + sum_{j != i} A[i,j] h1[b,j,:] + bias           (the diagonal term first, then j ascending, fmaf, fp32).
 * dhaug_graph_mix, transpose = 0: src = H (M, ld_src >= 2C), fp32 (src_bf16 = 0) or bf16 (1); bias C fp32 or NULL; dst = z, fp32
 *   (M, ld_dst >= C) or bf16 (M, ld_dst >= ceil16 C) with columns [C, ceil16 C) written as zeros (the next GEMM's operand).
 *   transpose = 1, the adjoint: src = g (M, ld_src >= C), dst = dH (M, ld_dst >= 2C; bf16: >= ceil16(2C), the pad written as zeros),
 *     dh0[b,i,:] = A[i,i] g[b,i,:],   dh1[b,j,:] = sum_{i != j} A[i,j] g[b,i,:]     (i ascending); bias must be NULL.
 *   The own row's term enters the off-diagonal sum with weight 0, as in the reference's dense products (it matters only to a row that
 *   holds inf or NaN).  One rounding on a bf16 output.  No column of a source row at or beyond 2C (C) is read, none of dst beyond the pad written.
 *   ALIGNMENT: none beyond the element's own.  The kernel takes 16-byte accesses only where it finds both bases, both pitches and
 *   C x element size on the 16-byte grid, and goes element by element otherwise (any C >= 1, e.g. the output layer's C = 3, ld 6).
 *   A and bias are read element by element always: they may lie on any 4-byte boundary (tensors of odd size in PosenetAdam's flat
 *   buffer).  No atomics: the same call gives the same bits.
 * dhaug_graph_adj_grad: the gradient of A.  g (M, ld_g >= C), h = H (M, ld_h >= 2C), each fp32 or bf16; pairs: device, nnz x (i, j)
 *   int32, 0 <= nnz <= DHAUG_GRAPH_MAX_PAIRS; dA: 16 x 16 fp32.  At every listed pair
 *     dA[i,j] = sum_{b,c} g[b,i,c] (i == j ? h0 : h1)[b,j,c],
 *   and EXACTLY 0 at every other entry (all 256 are written; a pair outside [0, 16) names no entry and is ignored).  Every product
 *   is formed and summed in fp64: per workgroup in a fixed order into workspace (device, DHAUG_GRAPH_ADJ_WORKSPACE_DOUBLES doubles,
 *   8-byte aligned; one call at a time per workspace), then a second launch adds the partials in workgroup order and rounds once.  No
 *   atomics: two calls give the same bits.  Element accesses only.
 * dhaug_graph_wcat: to_cat = 1: src = W (2, in, out) -> dst = Wcat (2 out, in), Wcat[k out + n, c] = W[k, c, n] (the B operand of
 *   H = x Wcat^T); to_cat = 0 the adjoint, src = dWcat -> dst = dW.  fp32, both contiguous, a copy (exact).  src != dst.
 * All three: DHAUG_EINVAL for a negative size, a flag outside {0, 1}, a NULL required pointer, M % 16 != 0, nnz outside its range;
 * DHAUG_EALIGN for a leading dimension below its minimum or a pointer off its element's grid; DHAUG_EUNSUPPORTED for C, in, out >= 2^28,
 * in x out >= 2^30; an empty problem (M = 0 or C = 0; in = 0 or out = 0) is a no-op that looks at no pointer. */
#define DHAUG_GRAPH_MIX_MAX_BLOCKS 512       /* workgroups of 256 items a mix launch takes at most: more items, more passes per thread */
#define DHAUG_GRAPH_MAX_PAIRS 256
#define DHAUG_GRAPH_ADJ_MAX_BLOCKS 64
#define DHAUG_GRAPH_ADJ_WORKSPACE_DOUBLES (DHAUG_GRAPH_ADJ_MAX_BLOCKS * DHAUG_GRAPH_MAX_PAIRS)
int dhaug_graph_mix(const void* src, int src_bf16, int64_t ld_src, const float* A, const float* bias, void* dst, int dst_bf16,
                    int64_t ld_dst, int64_t M, int64_t C, int transpose, void* stream);
int dhaug_graph_adj_grad(const void* g, int g_bf16, int64_t ld_g, const void* h, int h_bf16, int64_t ld_h, const int32_t* pairs,
                         int nnz, float* dA, void* workspace, int64_t M, int64_t C, void* stream);
int dhaug_graph_wcat(const float* src, float* dst, int64_t in, int64_t out, int to_cat, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * PoseFormer posenet: LayerNorm, short-sequence attention, exact GELU (R/models_baseline/poseformer/model_poseformer.py;
 * csrc/dhaug_attn.hip)
 * ----------------------------------------------------------------------------------------------------
 * Activations are rows; every tensor has a row pitch (ld, in elements).  A tensor with a *_bf16 flag is fp32 (0) or bf16 (1); an
 * output is rounded once from the fp32 result.  Arithmetic is fp32 (fp64 for the LayerNorm parameter gradients' column sums).  No
 * entry reads or writes a column at or beyond the stated width.  Vector stores, no atomics, every sum in a fixed order: two calls on
 * the same inputs give the same bits.
 * ALIGNMENT of a row tensor: base on 16 bytes (fp32) or 8 bytes (bf16), ld a multiple of 4: rows are read and written as 4-element
 *   vectors.  gamma, beta, mean, rstd, lse, dgamma, dbeta: 4 bytes (read and written element by element: parameters may lie on any
 *   4-byte boundary of PosenetAdam's flat buffer).  DHAUG_EALIGN otherwise, and for a pitch below the tensor's width.
 *
 * dhaug_layernorm_forward: x (M, ld_x >= C) -> y (M, ld_y >= C), y = (x - mean) * rstd * gamma + beta per row, rstd = 1 / sqrt(var +
 *   eps), var the mean of the squared CENTRED values (the row is held in registers: one read), mean = m0 + sum(x - m0) / C with m0 =
 *   sum(x) / C -- a constant row has mean = its constant and y = beta exactly; the centred values x - mean are centred once more
 *   (their own mean is what fp32 cannot hold of the row's: a row of 1 000 + N(0, 1e-3) keeps its variance).  mean, rstd: M fp32 each, written for the backward
 *   pass; either may be NULL (evaluation).  DHAUG_EUNSUPPORTED: C % 16 != 0 or C > DHAUG_LAYERNORM_MAX_COLS.
 * dhaug_layernorm_backward: from x, the cotangent g (M, ld_g >= C), gamma and the forward's mean and rstd:
 *     dx = rstd * (g gamma - mean_c(g gamma) - xhat mean_c(g gamma xhat)),  xhat = (x - mean) rstd      (dx NULL: not computed)
 *     dgamma[c] = sum_r g[r,c] xhat[r,c],  dbeta[c] = sum_r g[r,c]                                       (both NULL: not computed)
 *   The column sums run in fp64 in two stages: up to DHAUG_LAYERNORM_MAX_BLOCKS workgroups each walk a slice of the rows with
 *   DHAUG_LAYERNORM_PARTIAL_ROWS (C <= 32) or half as many row lanes per column and write their partials to workspace (device,
 *   DHAUG_LAYERNORM_WORKSPACE_DOUBLES(C) doubles, 8-byte aligned, one call at a time per workspace); a second launch adds them in
 *   workgroup order and rounds once.  M = 0 writes zeros.  The same limits on C.
 * dhaug_attn_forward: qkv (S N, ld_qkv >= 3C), C = H hd: the output of the qkv Linear for S sequences of N tokens, columns [0, C) q,
 *   [C, 2C) k, [2C, 3C) v, head h in columns [h hd, (h + 1) hd) of each third.  Per sequence and head P = softmax(scale q k^T) over
 *   the N keys (row maximum subtracted before exp: scores of any finite size give finite results), out[:, h hd ...] = P v, out
 *   (S N, ld_out >= C): the operand of the proj Linear.  lse (S H N fp32, [(s H + h) N + i], may be NULL): the rows' log-sum-exp of
 *   the scaled scores.  Keys are summed in ascending order.  DHAUG_EUNSUPPORTED (no launch): N outside [1, DHAUG_ATTN_MAX_TOKENS],
 *   hd outside [4, DHAUG_ATTN_MAX_HEAD_DIM] or hd % 4 != 0.  Any S, H >= 0 (0: a no-op that looks at no pointer).
 * dhaug_attn_backward: from qkv and the cotangent dout (S N, ld_dout >= C) of out: dqkv (S N, ld_dqkv >= 3C), all of columns [0, 3C)
 *   written -- dq, dk, dv each in its third: the incoming gradient of the qkv Linear as it stands.  P is never stored in global
 *   memory: the kernel forms it again exactly as the forward pass did (the same scores, their maximum, exp, the sum).  out and lse
 *   are checked like the other arguments and NOT read: exp(score - lse) would carry the rounding of lse (half an ulp of a number the
 *   size of the largest score: 4e-6 at scores of 80) into every weight, and D = dout . out would not cancel the rounding of dP where
 *   P is peaked; both were measured above the bound of tests/test_gpu_attn_kernels.py.
 *     dP_ij = dout_i . v_j,  D_i = sum_j P_ij dP_ij,  dS_ij = P_ij (dP_ij - D_i),  dq_i = scale sum_j dS_ij k_j,  dk_j = scale sum_i dS_ij q_i,
 *     dv_j = sum_i P_ij dout_i                                                              (j and i ascending).
 *   dqkv must not alias qkv (DHAUG_EINVAL).  The same limits.
 * dhaug_gelu_forward: y = z Phi(z), Phi the normal distribution function by erfc (the exact form, not tanh), z fp32 (M, ld_z >= C)
 *   -- the pre-activation a GEMM wrote, bias included -- y (M, ld_y >= C) fp32 or bf16.  Any C >= 1 (the C % 4 columns behind the last
 *   vector go element by element); M = 1 lifts the rule on the pitches.
 * dhaug_gelu_backward: dz = g (Phi(z) + z phi(z)), g (M, ld_g >= C) fp32 or bf16, dz fp32 or bf16.
 *   Both take at most DHAUG_GELU_MAX_BLOCKS workgroups of 256 four-column items: more items, more passes per thread.
 * All: DHAUG_EINVAL for a negative size, a flag outside {0, 1}, a NULL required pointer. */
#define DHAUG_LAYERNORM_MAX_COLS 2048
#define DHAUG_LAYERNORM_MAX_BLOCKS 256
#define DHAUG_LAYERNORM_PARTIAL_ROWS 8
#define DHAUG_LAYERNORM_WORKSPACE_DOUBLES(C) (2LL * DHAUG_LAYERNORM_MAX_BLOCKS * (C))
#define DHAUG_ATTN_MAX_TOKENS 81
#define DHAUG_ATTN_MAX_HEAD_DIM 64
#define DHAUG_ATTN_MAX_BLOCKS 8192
#define DHAUG_GELU_MAX_BLOCKS 2048
int dhaug_layernorm_forward(const void* x, int x_bf16, int64_t ld_x, const float* gamma, const float* beta, float eps, void* y,
                            int y_bf16, int64_t ld_y, float* mean, float* rstd, int64_t M, int64_t C, void* stream);
int dhaug_layernorm_backward(const void* x, int x_bf16, int64_t ld_x, const void* g, int g_bf16, int64_t ld_g, const float* gamma,
                             const float* mean, const float* rstd, void* dx, int dx_bf16, int64_t ld_dx, float* dgamma,
                             float* dbeta, void* workspace, int64_t M, int64_t C, void* stream);
int dhaug_attn_forward(const void* qkv, int qkv_bf16, int64_t ld_qkv, void* out, int out_bf16, int64_t ld_out, float* lse,
                       int64_t S, int N, int H, int hd, float scale, void* stream);
int dhaug_attn_backward(const void* qkv, int qkv_bf16, int64_t ld_qkv, const void* out, int out_bf16, int64_t ld_out,
                        const float* lse, const void* dout, int dout_bf16, int64_t ld_dout, void* dqkv, int dqkv_bf16,
                        int64_t ld_dqkv, int64_t S, int N, int H, int hd, float scale, void* stream);
int dhaug_gelu_forward(const float* z, int64_t ld_z, void* y, int y_bf16, int64_t ld_y, int64_t M, int64_t C, void* stream);
int dhaug_gelu_backward(const float* z, int64_t ld_z, const void* g, int g_bf16, int64_t ld_g, void* dz, int dz_bf16, int64_t ld_dz,
                        int64_t M, int64_t C, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Inverse kinematics of the DH skeleton (csrc/dhaug_ik.hip, csrc/dhaug_ik_math.h).  The reference has no counterpart: it
 * ships the plots of the dataset's angle distributions (my_draw_original_dataset_distribute_for_paper) but not the solver.
 * One lane owns one pose (dhaug_ik_track: one sequence); no atomics, the same call gives the same bits; fp32 throughout.
 *
 * dhaug_fk_jacobian: J (N,48,37), row 3 j + c = coordinate c of joint j of dhaug_fk_forward(out_joints = 16), column = angle
 *   slot, metres per degree: d p_j / d theta_k = (pi/180) z_k x (p_j - t_k) for the joints behind k.  It is the Jacobian with
 *   respect to the generator's 31 live slots: the columns of the six slots the generator pins to 0 (4, 9, 22, 23, 28, 33) are
 *   exact zeros (of these FK reads 23 and 28, whose value is taken as 0), and so are the columns of 27 and 32, which move
 *   no joint.  alpha = +-90 deg is taken as exact, as in dhaug_fk_backward.  The whole matrix is written (a fill, then the
 *   nonzero entries).  At most DHAUG_FK_JACOBIAN_MAX_BLOCKS workgroups of 64 poses; more poses, more trips.
 * dhaug_ik_fit: per pose, root = joint 0 (bit for bit), bone_len = the 15 joint distances of used_16key_15bone_len_table,
 *   and the angles by exactly `iters` Levenberg-Marquardt steps on r = FK16(theta, bone_len, root) - pose:
 *     (H + lambda diag(H) + 1e-8 I) delta = g,  H = J^T J, g = J^T r (Cholesky);  theta' = clamp(theta - delta, lo, hi);
 *     accepted when sum |r|^2 falls, then lambda *= 0.3, else theta stays and lambda *= 5;  lambda in [1e-9, 1e6].
 *   pose16 (N,16,3).  init (N,37) or NULL (T-pose) is clamped to the limits; lo / hi (37 each, device) or both
 *   NULL (the generator's limits).  angles (N,37): the six pinned slots are written as 0.  residual (N): the largest joint distance
 *   of the returned solution in metres.  DHAUG_EINVAL for iters < 1, lambda0 <= 0, only one of lo / hi.
 * dhaug_ik_track: the same over S concatenated sequences, frames seq_offset[s] .. seq_offset[s + 1] - 1 (S + 1 ascending int64 on
 *   the device, seq_offset[0] >= 0; the caller vouches for them: they address pose16 and every output).  Frame 0 of a sequence
 *   starts from init (S,37) or the T-pose, frame t from frame t - 1's solution; lambda starts at lambda0 in every frame.
 *   Parallel over sequences, serial inside one.
 * dhaug_ik_fit_staged: dhaug_ik_fit in S stages (coarse to fine), each under a per-joint weight w_j >= 0 on the residual:
 *     cost = sum_j w_j^2 |r_j|^2,  H = sum_j w_j^2 J_j^T J_j,  g = sum_j w_j^2 J_j^T r_j   (joints 1..15; the root has no term).
 *   stage_weights (S x 16, HOST, entry 0 of a row is checked but unused) and stage_iters (S, HOST) are read before the call
 *   returns and travel as kernel arguments: one table for the whole launch.  Stage s starts from where stage s - 1 stopped, with
 *   lambda back at lambda0 and the cost taken anew under its own weights, and runs exactly stage_iters[s] steps.  A joint of
 *   weight 0 adds exact zeros (its target must still be a finite number: 0 x NaN is NaN); an unknown that moves only such joints keeps its (clamped) start value bit for bit.  bone_len_in (N,15)
 *   replaces the closed-form lengths (a joint of weight 0 may be anywhere: it would spoil them), NULL = closed form.  residual:
 *   the largest joint distance over the joints of weight > 0 in the LAST stage.  One stage of weights 1.0 gives dhaug_ik_fit's
 *   bits.  DHAUG_EINVAL before any launch for S outside 1..8, a stage_iters below 1, a negative or non-finite weight (or square),
 *   a last stage whose weights are all 0, lambda0 <= 0, only one of lo / hi.
 * dhaug_ik_fit / dhaug_ik_fit_staged / dhaug_ik_track take at most DHAUG_IK_MAX_BLOCKS workgroups (two fit one CU: 69.25 KB of
 *   LDS each). */
#define DHAUG_FK_JACOBIAN_MAX_BLOCKS 1024
#define DHAUG_IK_MAX_BLOCKS 512
int dhaug_fk_jacobian(const float* angles, const float* bone_len, float* J, int64_t N, void* stream);
int dhaug_ik_fit(const float* pose16, const float* init, const float* lo, const float* hi, float* angles, float* bone_len,
                 float* root, float* residual, int64_t N, int iters, float lambda0, void* stream);
int dhaug_ik_fit_staged(const float* pose16, const float* init, const float* lo, const float* hi, const float* bone_len_in,
                        const float* stage_weights, const int* stage_iters, int S, float lambda0, float* angles, float* bone_len,
                        float* root, float* residual, int64_t N, void* stream);
int dhaug_ik_track(const float* pose16, const int64_t* seq_offset, const float* init, const float* lo, const float* hi,
                   float* angles, float* bone_len, float* root, float* residual, int64_t S, int iters, float lambda0,
                   void* stream);

/* ------------------------------------------------------------------------------------------------------
 * DOF angle distributions (csrc/dhaug_dof.hip, per-value arithmetic in csrc/dhaug_dof_math.h): the tables that
 * R/models_Fk_GAN/special_operate.py my_draw_DOF_angle_distribute :347-364 and my_draw_distribute_for_paper :420-442 build in
 * Python loops, accumulated on the device.  angles: fp32 (rows, D) with `pitch` >= D floats between rows, 1 <= D <=
 * DHAUG_DOF_MAX_SLOTS; D = 37 is generator_angle / IkFit.angles37, D = 33 the 'normal' sampler's table.
 *
 * Binning (both entries): bin = (int)truncf(a) + 180 of DHAUG_DOF_BINS = 361, the reference's int(angle) + 180: -0.5 -> 180 (bin
 *   180 is two degrees wide), 180.5 -> 360 and -180.9 -> 0, both inside.  |truncf(a)| > 180 or +-inf: counted in the end bin 0 or
 *   360 AND in `outside` (the reference wraps or raises there; this clamps and says so).  NaN: counted in `nan`, no bin.
 * Skip rule (both entries): with `residual` (rows fp32, NULL = none) a row whose residual > max_residual, or is NaN, is left out
 *   of everything and counted in `skipped`; residual == max_residual is kept.
 *
 * dhaug_dof_histogram accumulates into a caller-initialised record of DHAUG_DOF_RECORD_WORDS(D) 8-byte words:
 *   word DHAUG_DOF_OFF_ROWS     int64   rows seen (skipped ones included)
 *        DHAUG_DOF_OFF_SKIPPED  int64   rows left out by the skip rule
 *        DHAUG_DOF_OFF_NAN(D) + d, _OUTSIDE, _AT_LO, _AT_HI, _INF   int64 per slot d (inf: the +-inf among `outside`, so
 *                               that counts.sum() - inf is the number of values behind sum / sumsq)
 *        DHAUG_DOF_OFF_MIN(D) + d, _MAX    fp64 per slot: the exact fp32 extreme of the non-NaN values (infinities included; of
 *                               two zeros min keeps -0, max +0).  Initialise to +inf / -inf.
 *        DHAUG_DOF_OFF_SUM(D) + d, _SUMSQ  fp64 per slot: sum of a and of a * a (exact products) over the FINITE values
 *        DHAUG_DOF_OFF_COUNTS(D) + d * 361 + bin   int64
 *   per slot counts.sum() + nan == rows - skipped.  at_lo += a <= fl32(lo[d] + tol), at_hi += a >= fl32(hi[d] - tol), compared in
 *   fp32, with lo / hi (D each, device) both given or both NULL (then neither is counted).
 *   Layout: a workgroup of DHAUG_DOF_BLOCK lanes walks a slab of consecutive rows downwards, RG = DHAUG_DOF_BLOCK / D whole rows
 *   per step (lane l: slot l % D of row l / D of the step: one contiguous read), min / max / sum / sumsq in the lane's
 *   registers, counts in an LDS table of D x 361 uint32 (no-return LDS adds).  The partition depends on (rows, D) only:
 *   steps = ceil(rows / RG), slabs = min(DHAUG_DOF_MAX_BLOCKS, ceil(steps / DHAUG_DOF_MIN_STEPS)), steps per slab = ceil(steps /
 *   slabs).  A slab's non-zero counters are added to the record with no-return global INTEGER adds -- they commute exactly, so
 *   the counts are reproducible bits; the floating-point words never go through an atomic: every workgroup writes its four
 *   values per slot to `workspace` (DHAUG_DOF_WORKSPACE_BYTES) and a one-workgroup second launch folds them into the record in
 *   slab order.  The same call sequence gives the same bits in every word of the record.
 * dhaug_dof_pair_histogram: table int64 (npairs, 361, 361), table[p][bin(a_i)][bin(a_j)] += 1 for the slot pairs (i, j) =
 *   pairs[2 p], pairs[2 p + 1] (HOST ints, read before the call returns), npairs <= DHAUG_DOF_MAX_PAIRS.  A row with a NaN in
 *   either slot of a pair is left out of that pair.  One lane per row, no-return global integer adds (a table does not fit
 *   LDS); equal bins within a wave are not folded first.
 * Both: DHAUG_EINVAL for rows < 0, D outside 1..64, a NULL record / workspace / table, (rows > 0) NULL angles, pitch < D, exactly
 *   one of lo and hi, a pair index outside [0, D), npairs outside 0..4; DHAUG_EUNSUPPORTED for rows >= 2^31; DHAUG_EALIGN for a
 *   record, workspace or table off the 8-byte grid.  All checked before any launch; rows = 0 (or npairs = 0) launches nothing.
 *   No host read, no synchronisation; launches go to `stream` and can be captured.
 * dhaug_dof_record_layout (host only): words13 (HOST) <- the first word of rows, skipped, nan, outside, at_lo, at_hi, inf, min,
 *   max, sum, sumsq, counts and DHAUG_DOF_RECORD_WORDS(D), as THIS build of the library lays a record out: a binding checks its
 *   own arithmetic against it.  DHAUG_EINVAL for D outside 1..64 or a NULL pointer. */
#define DHAUG_DOF_BINS 361
#define DHAUG_DOF_MAX_SLOTS 64
#define DHAUG_DOF_MAX_PAIRS 4
#define DHAUG_DOF_BLOCK 256             /* lanes of a workgroup: DHAUG_DOF_BLOCK / D rows per step */
#define DHAUG_DOF_MAX_BLOCKS 512
#define DHAUG_DOF_MIN_STEPS 16
#define DHAUG_DOF_WORKSPACE_BYTES (DHAUG_DOF_MAX_BLOCKS * 4 * DHAUG_DOF_MAX_SLOTS * 8)
#define DHAUG_DOF_OFF_ROWS 0
#define DHAUG_DOF_OFF_SKIPPED 1
#define DHAUG_DOF_OFF_NAN(D) 2
#define DHAUG_DOF_OFF_OUTSIDE(D) (2 + (D))
#define DHAUG_DOF_OFF_AT_LO(D) (2 + 2 * (D))
#define DHAUG_DOF_OFF_AT_HI(D) (2 + 3 * (D))
#define DHAUG_DOF_OFF_INF(D) (2 + 4 * (D))
#define DHAUG_DOF_OFF_MIN(D) (2 + 5 * (D))
#define DHAUG_DOF_OFF_MAX(D) (2 + 6 * (D))
#define DHAUG_DOF_OFF_SUM(D) (2 + 7 * (D))
#define DHAUG_DOF_OFF_SUMSQ(D) (2 + 8 * (D))
#define DHAUG_DOF_OFF_COUNTS(D) (2 + 9 * (D))
#define DHAUG_DOF_RECORD_WORDS(D) (2 + 9 * (D) + (D) * DHAUG_DOF_BINS)
int dhaug_dof_record_layout(int64_t D, int64_t* words13);
int dhaug_dof_histogram(const float* angles, int64_t rows, int64_t D, int64_t pitch, const float* residual, float max_residual,
                        const float* lo, const float* hi, float tol, void* record, void* workspace, void* stream);
int dhaug_dof_pair_histogram(const float* angles, int64_t rows, int64_t D, int64_t pitch, const float* residual,
                             float max_residual, const int* pairs, int npairs, int64_t* table, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHAUG_H */
