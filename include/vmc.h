/*
 * vmc.h — C ABI of libvmc.so, the MI355X (gfx950) kernels under the ViMoCLIP hot path.
 *
 * The reference (MarcosRodrigoT/VIMO-CLIP) has no FFI: its hot path sits behind Python nn.Module /
 * function signatures and runs on stock PyTorch ATen ops.  Each entry point below replaces the ATen
 * op site(s) named in its comment (paths relative to the reference checkout; SURVEY.md §2b ids K0..K16; K17..K22 are this project's own).
 * The Python mirror of the reference interface (vimo_clip_amd/) calls these through ctypes.
 *
 * Conventions
 *   - plain pointers + sizes only; every buffer (inputs, outputs, workspace) is owned by the caller
 *     (PyTorch's allocator); kernels never allocate, free or retain pointers;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); no hidden streams,
 *     no device synchronisation, safe under hipGraph capture;
 *   - return 0 on success, a positive hipError_t on a HIP failure, a negative VMC_E_* on a bad argument;
 *     never throws, never aborts;
 *   - stateless and re-entrant; one process per GPU.
 *   - "16-bit" tensors are bf16 or f16, selected per call by `dtype16` (VMC_BF16 / VMC_F16); all
 *     reductions, softmax, LayerNorm statistics and GEMM accumulation are fp32.
 */
#ifndef VMC_H
#define VMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { VMC_F32 = 0, VMC_BF16 = 1, VMC_F16 = 2 };
enum { VMC_ACT_NONE = 0, VMC_ACT_QUICKGELU = 1, VMC_ACT_GELU_ERF = 2, VMC_ACT_RELU = 3 };
enum {
  VMC_E_ARG = -1,       /* null pointer / non-positive size */
  VMC_E_ALIGN = -2,     /* a stride or pointer violates the documented alignment */
  VMC_E_SHAPE = -3,     /* unsupported shape (e.g. K % 64 != 0, head_dim not supported) */
  VMC_E_DTYPE = -4
};

/* Library identity: returns the ABI version (1). */
int vmc_abi_version(void);
/* Human-readable message for a return code (static storage). */
const char* vmc_error_string(int code);
/* Diagnostics: `workgroups` workgroups of 256 threads run iters x 64 bf16 MFMAs and write {shader cycles (s_memtime), 100 MHz
 * ticks (s_memrealtime)} as two u64 each into out[2 * workgroups]: cycles / ticks x 100 MHz = the clock the chip sustains under an
 * MFMA load on THIS box (bench.py prints it beside the rooflines so that box-to-box swings of clock-sensitive kernels are visible). */
int vmc_clock_probe(void* out, int workgroups, int iters, int mfma_shape /* 0: 16x16x32, 1: 32x32x16 (same FLOPs per round) */, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K0 — frame preprocess + patch extraction.
 * Replaces the per-frame CPU loop  to_pil_image -> Resize/CenterCrop/ToTensor/Normalize
 * (models/student_model.py:77-78) and PIL + CLIPImageProcessor (extract_embeddings.py:89-93) for frames
 * that are already R x R (resize and crop are identities), and the im2col of visual.conv1
 * (models/student_model.py:84).
 *   frames  u8 [F,3,R,R] (NCHW, as FlowStudentModel.forward receives them)
 *   patches 16-bit [F*g*g, kpad], g = R/p, column k = c*p*p + dy*p + dx, columns >= 3*p*p zero
 *   value   ((wrap ? (256 - v) & 255 : v) / 255 - mean[c]) / std[c]   (wrap: SURVEY.md §7 quirk 1)
 */
int vmc_preprocess_patches_u8(const uint8_t* frames, void* patches, int F, int R, int p, int kpad,
                              int wrap_quirk, int dtype16, void* stream);

/* Same patch extraction for frames that are already normalised floats: `pixel_values` f32 [F,3,R,R], the
 * argument of CLIPModel.get_image_features (extract_embeddings.py:91-94). */
int vmc_patches_f32(const float* pixel_values, void* patches, int F, int R, int p, int kpad, int dtype16,
                    void* stream);

/* Split-precision patch operands for the INFERENCE patch-embedding GEMM (0.2 % of the encoder's FLOPs, but its 16-bit operand
 * rounding was the largest single term of the embedding error).  Same op sites as the two entries above.
 *   vmc_patches_u8_exact:  patches 16-bit [F*g*g, 2*kpad] = [v | v], v = the raw pixel 0..255 (exact in 16 bits; wrap_quirk as
 *     above).  Pair with W = [W'_hi | W'_lo], W'[n,k] = conv1[n,k] / std_c, bias'[n] = -255 sum_k conv1[n,k] mean_c / std_c and
 *     alpha = 1/255 in vmc_linear:  alpha (A W^T + bias') = sum_k ((v/255 - mean_c) / std_c) conv1[n,k]  to fp32 accuracy.
 *   vmc_patches_f32_split: patches [F*g*g, 3*kpad] = [x_hi | x_lo | x_hi], x_lo = x - x_hi; pair with W = [W_hi | W_hi | W_lo].
 * Columns >= 3 p^2 of every kpad-wide part are zero. */
int vmc_patches_u8_exact(const uint8_t* frames, void* patches, int F, int R, int p, int kpad, int wrap_quirk, int dtype16,
                         void* stream);
int vmc_patches_f32_split(const float* pixel_values, void* patches, int F, int R, int p, int kpad, int dtype16, void* stream);

/* Grey twins of vmc_preprocess_patches_u8 / vmc_patches_u8_exact for frames whose three channels are one plane (frame-difference
 * motion frames, vmc_frame_diff_gray_u8 below):  frames u8 [F,1,R,R], every other argument as the original.  `patches` receives the
 * bytes the original writes when given that plane three times (wrap_quirk, zeroed pad columns, bf16 / f16, even and odd p alike);
 * a third of the bytes are read.  The patch GEMM keeps its 3 p^2-deep K: folding the channels would change the sums' bits. */
int vmc_preprocess_patches_gray_u8(const uint8_t* frames, void* patches, int F, int R, int p, int kpad,
                                   int wrap_quirk, int dtype16, void* stream);
int vmc_patches_gray_u8_exact(const uint8_t* frames, void* patches, int F, int R, int p, int kpad, int wrap_quirk, int dtype16,
                              void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Frame-difference motion frames from RGB frames.
 * Replaces the host loop  cv2.cvtColor(frame, COLOR_BGR2GRAY) -> cv2.absdiff(curr, prev)  of
 * utils/generate_frame_diff_video.py:37-54 (the arithmetic before its lossy H.264 encode), whose output every *_frame_diff*
 * twin consumes as three identical channels.
 *   frames  u8, T RGB frames of H x W addressed by BYTE strides: element (t, c, y, x) at
 *           frames + t*stride_t + c*stride_c + y*stride_y + x*stride_x.  [T,H,W,3] (decoders), [T,3,H,W]
 *           (FlowStudentModel.forward) and permuted / sliced views of either need no copy.
 *   prev    NULL, or ONE frame that precedes frames[0] with the same stride_c / stride_y / stride_x (the previous chunk's
 *           last frame when a video is streamed in chunks)
 *   n_out   = T - 1 + (prev != NULL)
 *   gray(p) = (w_r*R + w_g*G + w_b*B + (1 << (shift-1))) >> shift
 *   out     u8 [n_out, channels_out, H, W] planar, contiguous:  out[t] = |gray(f[t+1]) - gray(f[t])|, f = (prev,) frames[0..T-1];
 *           channels_out is 1 or 3 (the plane is written three times)
 * Weights: 9798, 19235, 3735, shift 15 = OpenCV 4.x 8-bit COLOR_BGR2GRAY (parity unpinned: cv2 is absent here);
 * 4899, 9617, 1868, shift 14 = the 14-bit constants of other OpenCV builds.
 * VMC_E_ARG, before any launch: frames or out NULL, T / H / W <= 0, n_out <= 0, channels_out not 1 or 3, shift outside 1..22,
 * a negative weight, w_r + w_g + w_b != 1 << shift (the sum rule keeps gray <= 255).
 * HBM: 3 B read + channels_out B written per output pixel; 4-byte accesses per lane where 4 whole pixels sit at a 4-byte
 * aligned address (stride_x == 3 with stride_c == 1, or stride_x == 1), bytes elsewhere, the same result either way.  A thread
 * walks time and keeps the previous frame's grey values in registers; the outputs are split into time segments of at least
 * VMC_FRAME_DIFF_MIN_SEG frames only as far as the grid needs to fill the machine (csrc/frame_diff.hip). */
#define VMC_FRAME_DIFF_MIN_SEG 8
int vmc_frame_diff_gray_u8(const uint8_t* frames, const uint8_t* prev, uint8_t* out, int T, int H, int W,
                           long long stride_t, long long stride_c, long long stride_y, long long stride_x,
                           int w_r, int w_g, int w_b, int shift, int channels_out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Bilinear resize of u8 frames, bit-exact with the MammalNet student's data path: dataset_frame_diff_mn.py:82-91
 * (frames.float() / 255 -> F.interpolate(size, mode="bilinear", align_corners=False), aten's CPU kernels) and the to_pil_image that
 * follows in the student (pic.mul(255).byte()).  The operation order is part of the contract (DESIGN.md "Bilinear resize"):
 * float32 throughout, one rounding per operation, scale = (float)in / (float)out, src = fma(scale, d + 0.5, -0.5) clamped at 0,
 * p(v) = v / 255 correctly rounded, then one of aten's two recipes:
 *   VMC_RESIZE_SEPARABLE  row = fma(lx0, p0, lx1 * p1), out = fma(ly0, row0, ly1 * row1)            (its generic kernel)
 *   VMC_RESIZE_WEIGHTS4   w_yx = ly_y * lx_x, out = fma(w11, p11, fma(w10, p10, fma(w00, p00, w01 * p01)))   (its channels-last kernel)
 * aten (torch 2.10, AVX-512) runs the second on contiguous frames when OH + OW <= VMC_RESIZE_ATEN_SMALL, and for three-channel
 * frames whenever the process has ONE thread (a DataLoader worker); the first otherwise.  Neither flag = the choice aten makes in a
 * multi-threaded process: by output size.  q = (u8) trunc(out * 255) is the same for both.
 *   src      u8, F frames of C planes of H x W addressed by BYTE strides: element (f, c, y, x) at
 *            src + f*s_f + c*s_c + y*s_y + x*s_x.  [T,H,W,3] stacks and [F,C,H,W] tensors are read in place.
 *   dst      contiguous [F,C,OH,OW]: f32 `out` (what _resize_frames returns), or with VMC_RESIZE_U8 the u8 `q` (the pixels
 *            to_pil_image makes of it).  H == OH && W == OW needs no special case: p(v) as f32, v as u8, by either recipe.
 *   out_mode 0 (f32) or VMC_RESIZE_U8, optionally | one recipe flag.
 * VMC_E_ARG, before any launch: src or dst NULL, F / H / W / OH / OW < 1, C not 1 or 3, out_mode negative, with unknown bits or with
 * both recipe flags.  VMC_E_SHAPE: more than 2^31 - 1 blocks of 8 rows x 256 columns.
 * HBM: the source once + 4 B (f32) or 1 B (u8) per output sample; 16-byte / 4-byte stores where four outputs sit at an aligned
 * address, scalar stores of the same values elsewhere (csrc/resize_bilinear.hip). */
enum { VMC_RESIZE_U8 = 1, VMC_RESIZE_SEPARABLE = 2, VMC_RESIZE_WEIGHTS4 = 4 };
#define VMC_RESIZE_ATEN_SMALL 128
int vmc_resize_bilinear_u8(const uint8_t* src, void* dst, int F, int C, int H, int W, int OH, int OW,
                           long long s_f, long long s_c, long long s_y, long long s_x, int out_mode, void* stream);
/* out[i] = (u8)((int)trunc(x[i] * 255) & 255), the product rounded to f32 first: to_pil_image on a float picture.  Specified for
 * 0 <= x <= 255 (the reference's cast is undefined outside); [0,1] floats give their PIL pixels, integer-valued floats v give
 * (256 - v) mod 256, the wrap of SURVEY.md §7 quirk 1.  x f32 [n], out u8 [n].  VMC_E_ARG: x or out NULL, n < 1. */
int vmc_unit_f32_to_u8(const float* x, uint8_t* out, long long n, void* stream);

/* Pillow-exact antialiased resample of planar u8 images [planes, in_h, in_w] along one axis — the BICUBIC
 * ``Resize`` of clip._transform (models/student_model.py:77-78) and of CLIPImageProcessor (extract_embeddings.py:91),
 * both of which call PIL.Image.resize.  out pixel o (of the resampled axis) = clip8((2^21 + sum_t in[lo_o + t] *
 * coeffs[o*ksize + t]) >> 22) with (lo_o, n_o) = bounds[2o], bounds[2o+1]; tables are Pillow's precompute_coeffs in
 * 22-bit fixed point, computed by the host in float64.  Only outputs [out_first, out_first + out_count) are written
 * (the centre crop is fused): horizontal -> out [planes, in_h, out_count], vertical -> out [planes, out_count, in_w].
 * wrap_quirk applies v -> (256 - v) & 255 to the INPUT pixels (the student's float -> to_pil_image wrap). */
int vmc_resample_u8(const uint8_t* in, uint8_t* out, const int* bounds, const int* coeffs, int planes, int in_h, int in_w,
                    int out_first, int out_count, int ksize, int horizontal, int wrap_quirk, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K1/K3/K5/K6/K7/K9/K11-K14 — Linear layers:  C = epilogue(A @ W^T)   (MFMA, fp32 accumulate).
 * Replaces nn.Linear / F.linear / conv1-as-GEMM / `x @ proj` op sites: visual.conv1, attn.in_proj,
 * attn.out_proj, mlp.c_fc, mlp.c_proj, proj (OpenAI clip VisionTransformer, called at
 * models/student_model.py:84), ResidualMLP.fc1/fc2 (models/student_model.py:33), classification_head
 * (:55-59), nn.MultiheadAttention in/out projections, ffn.0/ffn.3, classifier.1/.4, projection_layer
 * (TFAM/models/AMO_CLIP.py:19-29,84,86).
 *   A [M,K] 16-bit row-major (row stride lda elements), W [N,K] 16-bit row-major (ldw)
 *   v = act(acc + bias[n]);  C[orow, n] = alpha * v + res[rrow, n]
 *   orow = out_row_group ? m + m / out_row_group + 1 : m      (patch rows -> token rows, class row skipped)
 *   rrow = res_row_mod  ? m % res_row_mod : orow              (positional-embedding broadcast)
 *   bias (f32 [N]) and res may be NULL; C and res are f32 or 16-bit (out_dtype / res_dtype).
 * Requirements: K % 64 == 0, N % 4 == 0; lda, ldw % 8 == 0; ldc, ldres % 4 == 0; 16-byte aligned bases.
 */
int vmc_linear(const void* A, const void* W, const float* bias, const void* res, void* C,
               int M, int N, int K, int lda, int ldw, int ldc, int ldres,
               int act, float alpha, int out_dtype, int res_dtype, int out_row_group, int res_row_mod,
               int dtype16, void* stream);
/* vmc_linear with a side output for training: Z[m, n] (16-bit, row stride ldz >= N, ldz % 4 == 0, 16-byte aligned) receives
 * A W^T + bias BEFORE the activation, from the same epilogue that writes C = alpha * act(.) (+ res) -- the tensor the backward
 * of an activation needs (autograd of the QuickGELU / GELU linears, models/student_model.py:27-34, clip model.py MLP), without
 * a second pass over the 4D-wide matrix.  Z == NULL: identical to vmc_linear.  Not combined with out_row_group. */
int vmc_linear_preact(const void* A, const void* W, const float* bias, const void* res, void* C, void* Z,
                      int M, int N, int K, int lda, int ldw, int ldc, int ldres, int ldz,
                      int act, float alpha, int out_dtype, int res_dtype, int out_row_group, int res_row_mod,
                      int dtype16, void* stream);

/* Weight-gradient form of vmc_linear (autograd of F.linear w.r.t. the weight, train.py:104): C [M,N] f32 contiguous =
 * A [M,K] @ W [N,K]^T with a long contraction K (the token count) and a small output.  128x128 tiles x K slices; every
 * slice writes a partial slab into the workspace, a second kernel sums the slabs in a fixed order (deterministic).
 * K % 64 == 0, N % 4 == 0, lda/ldw % 8 == 0; workspace >= vmc_linear_splitk_workspace_bytes (may be 0 -> NULL). */
size_t vmc_linear_splitk_workspace_bytes(int M, int N, int K);
int vmc_linear_splitk_f32(const void* A, const void* W, float* C, int M, int N, int K, int lda, int ldw, void* workspace,
                          size_t workspace_bytes, int dtype16, void* stream);

/* Weight gradient straight from the token-major operands the forward left behind (no transposed copies):
 * C [N,K] f32 contiguous = dY[M,N]^T @ X[M,K], contraction over the M tokens (any M; rows past M read as zeros).
 * Both MFMA operands come from [64 tokens][128 columns] LDS tiles through ds_read_b64_tr_b16.  Token range split in
 * slices -> slabs in the workspace + deterministic reduce.  N % 8 == 0, K % 8 == 0, lddy/ldx % 8 == 0. */
size_t vmc_linear_wgrad_tn_workspace_bytes(int M, int N, int K);
int vmc_linear_wgrad_tn(const void* dY, const void* X, float* C, int M, int N, int K, int lddy, int ldx, void* workspace,
                        size_t workspace_bytes, int dtype16, void* stream);
/* Same launch, plus the bias gradient dbias[N] = column sums of dY (f32, 16-byte aligned; NULL = vmc_linear_wgrad_tn):
 * the dY fragments already in registers go through four more MFMAs against a ones operand, replacing a separate
 * column-sum pass over dY (autograd of F.linear's bias, train.py:104). */
int vmc_linear_wgrad_bias_tn(const void* dY, const void* X, float* C, float* dbias, int M, int N, int K, int lddy, int ldx,
                             void* workspace, size_t workspace_bytes, int dtype16, void* stream);

/* Many TN weight gradients in ONE launch (the weight gradients of a training step: TFAM/train_and_eval.py:94-95, train.py:103-104 --
 * `loss.backward()` leaves one small dW = dY^T X per linear).  Every 256 x 256 tile runs over all M tokens of its problem: no token
 * slices, no workspace, no reduce launch.  Per problem: M % 128 == 0 and M >= 256, N % 8 == 0, K % 8 == 0, lddy / ldx % 8 == 0,
 * operands < 2 GiB, pointers 16-byte aligned; C [N, K] f32 contiguous, dbias [N] f32 or NULL (column sums of dY).  n <= VMC_WGRAD_GROUP_MAX. */
#define VMC_WGRAD_GROUP_MAX 32
typedef struct vmc_wgrad_tn_problem {
  const void* dY;      /* [M, lddy] 16-bit */
  const void* X;       /* [M, ldx] 16-bit */
  float* C;            /* [N, K] */
  float* dbias;        /* [N] or NULL */
  int M, N, K, lddy, ldx, reserved;
} vmc_wgrad_tn_problem;
int vmc_linear_wgrad_tn_group(const vmc_wgrad_tn_problem* probs, int n, int dtype16, void* stream);

/* vmc_linear with the large-problem kernel chosen PER CALL (A/B measurements in one process; the library keeps no
 * state): VMC_GEMM_TWOSTAGE = two-stage tiles only, VMC_GEMM_DEFAULT = what vmc_linear does (8-phase 256x256 kernel; the
 * tile rows of a small last partial round handed to the small-tile kernel in a second launch; whole-tile problems with a
 * bias and a 16-bit output walk their tiles in a persistent workgroup per CU that prefetches the next tile's operands),
 * VMC_GEMM_NO_TAIL_SPLIT = the same without that split, VMC_GEMM_PERSISTENT = the same as VMC_GEMM_DEFAULT (kept for the
 * ABI), VMC_GEMM_ONE_TILE = never persistent (one tile per workgroup).  Results are identical bit for bit across them.
 * The routing of every variant is vimo_clip_amd/csrc/gemm_route.h. */
enum { VMC_GEMM_TWOSTAGE = 0, VMC_GEMM_DEFAULT = 1, VMC_GEMM_NO_TAIL_SPLIT = 2, VMC_GEMM_PERSISTENT = 3, VMC_GEMM_ONE_TILE = 4,
       VMC_GEMM_MFMA32 = 5, /* the persistent walk on v_mfma_f32_32x32x16 fragments (bias / QuickGELU / bias-free epilogues); the
                               k-steps are summed 16 at a time, so the last bit may differ from the other variants */
       VMC_GEMM_VARIANTS = 6 };
int vmc_linear_variant(const void* A, const void* W, const float* bias, const void* res, void* C,
                       int M, int N, int K, int lda, int ldw, int ldc, int ldres,
                       int act, float alpha, int out_dtype, int res_dtype, int out_row_group, int res_row_mod,
                       int dtype16, int variant, void* stream);

/* 16-bit 2-D transpose  out[c, r] = in[r, c]  (rows x cols, element strides ld_in / ld_out); used for
 * the dgrad/wgrad operand layouts of K8 (autograd of F.linear, train.py:104). */
int vmc_transpose16(const void* in, void* out, int rows, int cols, int ld_in, int ld_out, void* stream);

/* f32 -> 16-bit cast of a weight matrix [rows, cols] (+ optional transposed copy [cols, rows]); the
 * 16-bit compute copies of the fp32 master parameters (models/student_model.py:45 keeps fp32). */
int vmc_cast_weight(const float* w, void* w16, void* w16_t, int rows, int cols, int ld_out, int ld_out_t,
                    int dtype16, void* stream);

/* The same for many weights in ONE launch: after an optimiser step (`optimizer.step()`, train.py:107, TFAM/train_and_eval.py:96)
 * every 16-bit compute copy of the trained parameters is refreshed in place.  `desc` is a DEVICE array of n_desc records of
 * 48 bytes {const float* w; void* w16; void* w16_t; int rows, cols, ld_out, ld_out_t, tile0, tiles_x;} (NULL copies are skipped);
 * record i owns the 64x64 tiles [tile0, tile0 of record i+1) of a 1-D grid of total_tiles, tiles_x = ceil(cols / 64).
 * 16-byte loads and 8-byte stores where a record's w is 16-byte aligned, its copies 8-byte aligned and rows, cols, ld_out and
 * ld_out_t are multiples of 4; scalar accesses for a record where they are not (neither is an error). */
int vmc_cast_weights_multi(const void* desc, int n_desc, int total_tiles, int dtype16, void* stream);

/* Column sums  out[n] = sum_m in[m, n]  (bias gradients, K8).  N % 4 == 0, ld_in % 4 == 0.  workspace: >= vmc_colsum_workspace_bytes. */
size_t vmc_colsum_workspace_bytes(int M, int N);
int vmc_colsum(const void* in, float* out, int M, int N, int ld_in, int in_dtype, void* workspace,
               size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K2 — LayerNorm (eps inside sqrt, fp32 statistics).  Replaces ln_pre/ln_1/ln_2/ln_post of the CLIP
 * ViT and norm_self/norm_cross/norm_ffn/classifier.0 (TFAM/models/AMO_CLIP.py:32-34,84).
 *   x [rows, D] (row stride ldx; f32 or 16-bit), gamma/beta f32 [D]
 *   y16 (16-bit, ld = D) and/or y32 (f32, ld = D): either may be NULL
 *   mean/rstd f32 [rows]: optional saves for the backward
 * Requirements: D % 4 == 0, D <= 4096.
 */
int vmc_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y16, float* y32,
                      float* mean, float* rstd, int rows, int D, int ldx, float eps, int x_dtype,
                      int dtype16, void* stream);
/* Fused residual update + LayerNorm of the pre-LN ViT blocks: x (fp32 residual stream, row stride ldx) <- x +
 * branch (16-bit attention / MLP branch output, row stride ldb), written back when write_x != 0, and
 * y16 [rows, D] = LN(x).  Replaces `x = x + attn(...)` / `x = x + mlp(...)` followed by ln_2 / the next ln_1 /
 * ln_post (OpenAI clip ResidualAttentionBlock.forward).  D % 256 == 0, D <= 2048. */
int vmc_add_layernorm_fwd(float* x, const void* branch, const float* gamma, const float* beta, void* y16, int rows,
                          int D, int ldx, int ldb, float eps, int write_x, int dtype16, void* stream);

/* The same with TWO 16-bit branches, x <- (x + branch0) + branch (in that order) and y16 = LN(x).  Lets the first add+LayerNorm of
 * a pre-norm block (after out_proj; x = x + attention(...), modeling_clip.py / OpenAI clip ResidualAttentionBlock.forward) skip
 * writing the fp32 stream back (write_x = 0) and the second one (after c_proj) redo that add from the kept attention branch:
 * 22 instead of 24 bytes per element and layer, bit-identical stream. */
int vmc_add2_layernorm_fwd(float* x, const void* branch0, const void* branch, const float* gamma, const float* beta, void* y16,
                           int rows, int D, int ldx, int ldb0, int ldb, float eps, int write_x, int dtype16, void* stream);
/* Post-norm block tail of the TFAM AttentionLayer (TFAM/models/AMO_CLIP.py:40,45,50: norm(x + dropout(branch))):
 * s = x (f32 [rows,D]) + branch (16-bit [rows,D]); y = LN(s) written as f32 (y32, next residual operand) and/or 16-bit
 * (y16, next GEMM operand); optional saves for the backward: sum_out = s, mean, rstd.  D % 256 == 0, D <= 2048. */
int vmc_postnorm_fwd(const float* x, const void* branch, const float* gamma, const float* beta, float* sum_out, float* y32,
                     void* y16, float* mean, float* rstd, int rows, int D, float eps, int dtype16, void* stream);
/* The same tail with the branch passed through one or two dropouts first: LN(x + drop2(drop1(branch))) -- the FFN's trailing
 * nn.Dropout and the block's own dropout (AMO_CLIP.py:28,50; :40,45 for the attention tails).  Masks are vmc_dropout's
 * counter-based masks on the flat element index (same seed -> same mask), so the backward can regenerate them.
 * drop_p2 > 0 requires drop_p1 > 0. */
int vmc_postnorm_dropout_fwd(const float* x, const void* branch, const float* gamma, const float* beta, float* sum_out, float* y32,
                             void* y16, float* mean, float* rstd, int rows, int D, float eps, float drop_p1,
                             uint64_t drop_seed1, float drop_p2, uint64_t drop_seed2, int dtype16, void* stream);
/* Backward (autograd of the LayerNorms, train.py:104): dx [rows,D] (f32 or 16-bit per dx_dtype) =
 * LN'(dy) + add, where `add` (optional, dx's dtype/layout) is the gradient arriving over the residual
 * branch that forks at x (fused so the fork needs no separate add pass).  dgamma/dbeta f32 [D],
 * overwritten.  dy f32 or 16-bit.  D <= 2048. */
size_t vmc_layernorm_bwd_workspace_bytes(int rows, int D);
int vmc_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                      const void* add, void* dx, float* dgamma, float* dbeta, int rows, int D, int ldx,
                      int dy_dtype, int x_dtype, int dx_dtype, int dtype16, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The same with TWO incoming gradients dy + dy2 (dy2 16-bit [rows, D], may be NULL): a post-norm LayerNorm output feeds both the fp32
 * residual path and the 16-bit GEMM operand of the next sub-layer (AMO_CLIP.py:40-50), so its backward receives one gradient of each
 * type; summed in fp32 inside the kernel (was: a separate add pass). */
int vmc_layernorm_bwd2(const void* dy, const void* dy2, const void* x, const float* gamma, const float* mean, const float* rstd,
                       const void* add, void* dx, float* dgamma, float* dbeta, int rows, int D, int ldx,
                       int dy_dtype, int x_dtype, int dx_dtype, int dtype16, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Backward of vmc_postnorm_dropout_fwd in one launch (+ the partial reduce of dgamma / dbeta): with the saved pre-norm sum, mean and rstd,
 *   dsum (f32 [rows, D])       = LayerNorm'(dy + dy2)            (dy f32 or 16-bit, dy2 16-bit or NULL, as vmc_layernorm_bwd2)
 *   dbranch16 (16-bit [rows, D]) = cast(dsum * mask1/(1-p1) * mask2/(1-p2))   (the forward's masks, regenerated from the seeds)
 * i.e. what vmc_layernorm_bwd2 followed by vmc_cast_dropout2 (p = 0: a plain cast) computes, bit for bit, without the second pass over
 * the gradient (autograd of `norm(x + dropout(branch))`, TFAM/models/AMO_CLIP.py:40-50 under TFAM/train_and_eval.py:83). */
int vmc_postnorm_bwd(const void* dy, const void* dy2, const float* sum, const float* gamma, const float* mean, const float* rstd,
                     float* dsum, void* dbranch16, float* dgamma, float* dbeta, int rows, int D, int dy_dtype, float p1,
                     uint64_t seed1, float p2, uint64_t seed2, int dtype16, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K4 — ViT self-attention  softmax(Q K^T / sqrt(dh)) V, no mask, head_dim 64 (MFMA).
 * Replaces the SDPA inside nn.MultiheadAttention of every CLIP residual block.
 *   qkv 16-bit [F*N, 3*D] packed as the in_proj output: columns [0,D)=Q, [D,2D)=K, [2D,3D)=V, head h at
 *   columns h*64..h*64+63;  out 16-bit [F*N, D].   D = H*64, any N >= 1: N <= 288 keeps a head's K/V in LDS,
 *   longer sequences (ViT-L/14@336px: N = 577) stream 64-key K/V tiles through LDS.
 *   lse f32 [F, H, N] optional (log-sum-exp of the scaled scores, saved for the backward).
 */
int vmc_attention_vit_fwd(const void* qkv, void* out, float* lse, int F, int N, int H, int dtype16,
                          void* stream);

/* The same attention for the CLASS-TOKEN query only: what the last residual block of the encoder needs (only x[:, 0] reaches
 * ln_post: `x = self.ln_post(x[:, 0, :])`, OpenAI clip model.py; modeling_clip.py:650 pooled_output = last_hidden_state[:, 0]).
 *   q_cls 16-bit [F, D] (the class rows' queries), kv 16-bit [F*N, 2*D] (columns [0,D)=K, [D,2D)=V of every token),
 *   out 16-bit [F, D].  Any N >= 1.  N <= 288: same kernel, one 16-row query tile per (frame, head) instead of ceil(N/16);
 *   longer: one wave per (frame, head) through the key tiles of the streamed kernel.  Either way the class row equals row 0
 *   of vmc_attention_vit_fwd bit for bit. */
int vmc_attention_vit_cls_fwd(const void* q_cls, const void* kv, void* out, int F, int N, int H, int dtype16, void* stream);

/* K4/K11/K12 generic masked attention, any head_dim <= 128 with head_dim % 8 == 0.
 * Replaces F.multi_head_attention_forward's core (q*dh^-1/2, key_padding_mask -> -inf, softmax, @V)
 * for the TFAM self/cross attention (TFAM/models/AMO_CLIP.py:39-45) and serves as the backward's
 * forward-recompute reference.
 *   head_dim 64 / 96: MFMA kernels with NO length limit (Tk <= 64: one wave per (b, h); longer: tiled kernels
 *   streaming 64-key tiles with an online softmax); other head dims: fp32 scalar kernels, Tq, Tk <= 2048
 *   (VMC_E_SHAPE beyond).  The tiled kernels also need out 8-byte aligned; otherwise the scalar kernel runs.
 *   q  16-bit, element (b, t, h, d) at q[(b*Tq + t)*ldq + h*dh + d];  k, v likewise with Tk, ldk, ldv
 *   key_mask u8 [B, Tk], 1 = attend, 0 = padding (the reference's mask_rgb/mask_flow), may be NULL
 *   out 16-bit [(b*Tq+t)*ldo + h*dh + d];  lse f32 [B,H,Tq] optional.
 *   A query row whose keys are all masked yields NaN, as torch does.
 *   dropout_p > 0 drops attention probabilities after the softmax (nn.MultiheadAttention(dropout=p), train
 *   mode) with the counter-based keep mask hash(dropout_seed, ((b*H+h)*Tq+t)*Tk+key); the backward must be
 *   given the same (p, seed).
 */
int vmc_attention_fwd(const void* q, const void* k, const void* v, const uint8_t* key_mask, void* out,
                      float* lse, int B, int H, int Tq, int Tk, int dh, int ldq, int ldk, int ldv, int ldo,
                      float dropout_p, uint64_t dropout_seed, int dtype16, void* stream);
/* Backward of the above (autograd of the MHA core, train.py:104 / TFAM/train_and_eval.py:82): dq, dk, dv
 * 16-bit with their own row strides, fully overwritten.  workspace >= vmc_attention_bwd_workspace_bytes.
 *   head_dim 64 / 96 with lddq, lddk, lddv, ldo % 4 == 0: MFMA, no length limit (Q, K, V, dO of a head in LDS when they fit
 *   in 160 KB; longer: tiled two-pass kernels, no atomics, deterministic; these also need dq, dk, dv 8-byte and out 16-byte
 *   aligned); otherwise fp32 scalar kernels, Tq, Tk <= 2048. */
size_t vmc_attention_bwd_workspace_bytes(int B, int H, int Tq);
int vmc_attention_bwd(const void* q, const void* k, const void* v, const uint8_t* key_mask, const void* out,
                      const void* dout, const float* lse, void* dq, void* dk, void* dv,
                      int B, int H, int Tq, int Tk, int dh, int ldq, int ldk, int ldv, int ldo,
                      int lddq, int lddk, int lddv, float dropout_p, uint64_t dropout_seed, void* workspace,
                      size_t workspace_bytes, int dtype16, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Small element-wise / pooling pieces.
 */
/* rows[f*row_stride + 0..D) = a[0..D) + b[0..D)  for f < F  (class token + positional_embedding[0]). */
int vmc_set_class_rows(void* x, const float* a, const float* b, int F, int D, size_t row_stride, int x_dtype,
                       int dtype16, void* stream);
/* y = act(x) and dx = dy * act'(x) on [n] elements (training path keeps pre-activations). */
int vmc_act_fwd(const void* x, void* y, size_t n, int act, int dtype16, void* stream);
int vmc_act_bwd(const void* x, const void* dy, void* dx, size_t n, int act, int dtype16, void* stream);
/* out[b, :] = mean_t x[b, t, :]  over ALL T rows (TFAM/models/AMO_CLIP.py:170 pools padded rows too;
 * models/student_model.py:93).  x f32 or 16-bit, out16 and/or out32. */
int vmc_mean_pool(const void* x, void* out16, float* out32, int B, int T, int D, int x_dtype, int dtype16,
                  void* stream);
/* The same over the first n = *pool_len rows of every clip (see "POOL LENGTH" below; the row stride stays T):
 * out[b, :] = (1/n) sum_{t<n} x[b, t, :].  pool_len == NULL: vmc_mean_pool (which is this entry with NULL). */
int vmc_mean_pool_len(const void* x, void* out16, float* out32, int B, int T, int D, const int* pool_len, int x_dtype,
                      int dtype16, void* stream);
/* x[b,t,:] += pe[t,:]  sinusoidal positional encoding of TFAM/models/AMO_CLIP.py:88-97 (f32 in place). */
int vmc_add_sinusoidal_pe(float* x, int B, int T, int D, void* stream);
/* y = a + alpha * b elementwise, f32. */
int vmc_axpby_f32(const float* a, const float* b, float* y, size_t n, float alpha, float beta, void* stream);
/* y = a + b on flat arrays (sum of the two gradients meeting where a tensor is used twice; autograd of
 * the residual forks, train.py:104); each operand f32 or 16-bit. */
int vmc_add(const void* a, const void* b, void* y, size_t n, int a_dtype, int b_dtype, int y_dtype, int dtype16,
            void* stream);
/* Backward of vmc_mean_pool: dx[b,t,:] = dout[b,:] / T. */
int vmc_mean_pool_bwd(const void* dout, void* dx, int B, int T, int D, int dout_dtype, int dx_dtype, int dtype16,
                      void* stream);
/* Backward of vmc_mean_pool_len: dx[b,t,:] = dout[b,:] / n for t < n and 0 for n <= t < T (every row of dx is written). */
int vmc_mean_pool_bwd_len(const void* dout, void* dx, int B, int T, int D, const int* pool_len, int dout_dtype, int dx_dtype,
                          int dtype16, void* stream);
/* Training-path token assembly of K1 (class token concat + positional embedding, OpenAI clip
 * VisionTransformer.forward): x[f,0,:] = cls + pos[0]; x[f,1+p,:] = xp[f*(N-1)+p,:] + pos[1+p].
 * xp 16-bit [F*(N-1), D]; cls f32 [D]; pos f32 [N,D]; x [F*N, D] f32 or 16-bit. */
int vmc_assemble_tokens(const void* xp, const float* cls, const float* pos, void* x, int F, int N, int D,
                        int x_dtype, int dtype16, void* stream);
/* Inverted dropout, y = x * keep/(1-p), keep(i) = hash(seed, i) >= p (nn.Dropout of
 * TFAM/models/AMO_CLIP.py:27-35,84).  Stateless: the backward applies the same call to dy. */
int vmc_dropout(const void* x, void* y, size_t n, float p, uint64_t seed, int x_dtype, int dtype16, void* stream);
/* y16 = cast(x * mask1/(1-p1) * mask2/(1-p2)) in one pass (p = 0 skips a mask): the backward of vmc_postnorm_dropout_fwd's branch,
 * i.e. of `x + self.dropout(branch)` / the FFN's two trailing dropouts (AMO_CLIP.py:28,40,45,50), with the cast to the branch's type. */
int vmc_cast_dropout2(const float* x, void* y16, size_t n, float p1, uint64_t seed1, float p2, uint64_t seed2, int dtype16,
                      void* stream);
/* y = x * scale[0], the scale read from device memory (the scalar gradient arriving at a loss node). */
int vmc_scale_by_device_scalar(const float* x, float* y, size_t n, const float* scale, void* stream);
/* f32 <-> 16-bit casts on flat arrays. */
int vmc_cast_f32_to_16(const float* x, void* y, size_t n, int dtype16, void* stream);
int vmc_cast_16_to_f32(const void* x, float* y, size_t n, int dtype16, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K10 — losses (forward value + gradient in one pass, fp32).
 * Cosine / MSE distillation: losses.py:5-44.   student, teacher f32 [rows, E] (teacher row stride ldt
 * covers the `rgb_emb[:, :-1]` slice of train.py:98 via teacher_rows_per_clip / teacher_clip_stride).
 *   loss f32[1] (overwritten), dstudent f32 [rows,E] = d loss / d student (may be NULL).
 */
size_t vmc_loss_workspace_bytes(int rows);
int vmc_distill_loss(const float* student, const float* teacher, float* loss, float* dstudent,
                     int rows, int E, int rows_per_clip, size_t teacher_clip_stride, int mode_cosine,
                     void* workspace, size_t workspace_bytes, void* stream);
/* BCE-with-logits, pos_weight = pw*y + 1 (losses.py:59-67; pw < 0 means "None" -> weight 1; also
 * nn.BCEWithLogitsLoss of TFAM/train_and_eval.py:58).  logits/targets f32 [n]; mean over n.
 * dlogits = [(1 - y) sigmoid(x) - w y sigmoid(-x)] / n with w = pw*y + 1, each sigmoid formed without a subtraction: every
 * element keeps its relative accuracy in both confident tails. */
int vmc_bce_loss(const float* logits, const float* targets, float* loss, float* dlogits, int n, float pos_weight,
                 void* workspace, size_t workspace_bytes, void* stream);
/* Softmax cross entropy, mean over rows — nn.CrossEntropyLoss() of the MammalNet (single-label) variants:
 * train_frame_diff_mn.py:82,102 passes class indices (``labels.argmax(dim=1)``), TFAM/train_and_eval_frame_diff_MN.py:59,83
 * passes the float one-hot rows themselves (probability targets).  Exactly one of target_index (int64 [rows]) and
 * target_prob (f32 [rows,C]) is non-NULL.  logits f32 [rows,C]; loss f32[1]; dlogits f32 [rows,C] or NULL;
 * workspace >= vmc_loss_workspace_bytes(rows).
 * A row's loss is sum(y) log(sum exp(x - m)) - sum_c y_c (x_c - m), m = max x: accurate relative to log C and the loss itself,
 * whatever the size of the logits.  dlogits = (softmax(x) sum(y) - y) / rows. */
int vmc_cross_entropy_loss(const float* logits, const long long* target_index, const float* target_prob, float* loss,
                           float* dlogits, int rows, int C, void* workspace, size_t workspace_bytes, void* stream);

/* Contrastive (symmetric InfoNCE) distillation over the in-batch similarity matrix (not in the reference).
 * M rows (frames) of E columns, clip(i) = i / rows_per_clip; pair (i, j) is valid when clip(j) != clip(i) or j == i.
 *   u_i = s_i / max(|s_i|, 1e-5), v_j likewise, both rounded to the 16-bit type;  z = (1 / tau) u16 v16^T   (vmc_linear);
 *   loss = 1/(2M) sum_i [ lse_{j valid} z_ij - z_ii + lse_{j valid} z_ji - z_ii ];  dz = p_row + p_col - 2 I on valid pairs;
 *   du = dz16 v16 / (2 M tau)   (vmc_linear, A = dz16, W = v16^T);  ds through the normalisation.
 * Mp = M rounded up to 64 is the leading dimension of v16^T and dz16 and the row count of u16 / v16: what vmc_linear's K % 64 == 0
 * asks for.  1 <= M <= 16384 and E % 64 == 0, VMC_E_SHAPE otherwise.  Every argument is a shape constant and nothing is read
 * back: the chain can be captured into a graph.  The same input gives the same bits (fixed-order reductions, no atomics).
 *
 * vmc_contrastive_workspace_layout: byte offsets (host array of 9) of u16, v16, v16^T, z [M, Mp] f32, dz16 [M, Mp], lse_row [M],
 *   lse_col [M] and the softmax partials inside one workspace, each on a 256-byte boundary, and the total in offsets[8] (what
 *   vmc_contrastive_workspace_bytes returns; 0 for an unsupported shape).  vmc_contrastive_partials_bytes(M): the partials alone.
 * vmc_contrastive_prep: student f32 [M, E] dense; teacher f32 rows read through rows_per_clip (>= 1) / teacher_clip_stride exactly
 *   as vmc_distill_loss reads them.  Writes u16, v16 [Mp, E] (pad rows zero), vt16 [E, Mp] = the bits of v16 transposed (pad columns
 *   zero) and inv_s [M] = 1 / max(|s_i|, 1e-5).  The three 16-bit buffers are 16-byte aligned (VMC_E_ALIGN).  Two launches.
 * vmc_contrastive_softmax: z f32 [M, ldz], ldz >= M; only the first M columns of a row are read.  rows_per_clip >= 0, 0 = no mask.
 *   Writes lse_row, lse_col [M] (max-subtracted log-sum-exp over the valid entries of row i / column j), loss f32[1], top1 int32[1]
 *   (rows with z_ii >= z_ij for every valid j) and, unless dz16 is NULL, dz16 [M, Mp] with the pad columns zero.  The diagonal stays
 *   out of every running sum and is added last, so -log p_ii and dz_ii keep their relative accuracy where p_ii is near 1.
 *   Three launches, four with dz16.
 * vmc_contrastive_norm_bwd: du f32 [M, E], student, inv_s -> dstudent = inv_s (du - u (u . du)) where |s| > 1e-5 and du / 1e-5 where
 *   the clamp holds the norm.  dstudent may be du itself. */
size_t vmc_contrastive_workspace_bytes(int M, int E);
size_t vmc_contrastive_partials_bytes(int M);
int vmc_contrastive_workspace_layout(int M, int E, size_t* offsets);
int vmc_contrastive_prep(const float* student, const float* teacher, void* u16, void* v16, void* vt16, float* inv_s, int M, int E,
                         int rows_per_clip, size_t teacher_clip_stride, int dtype16, void* stream);
int vmc_contrastive_softmax(const float* z, int M, int ldz, int rows_per_clip, float* lse_row, float* lse_col, float* loss, int* top1,
                            void* dz16, int dtype16, void* partials, size_t partials_bytes, void* stream);
int vmc_contrastive_norm_bwd(const float* du, const float* student, const float* inv_s, float* dstudent, int M, int E, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K11-K14 fused — the TFAM forward as a chain of weight-streaming launches for short clips (T, Tk <= 64,
 * d_model 512 / 768, head_dim 64 / 96; vmc_tfam_supported): AttentionLayer.forward (TFAM/models/AMO_CLIP.py:37-51) in 6 launches
 * with the LayerNorms, both attentions, bias / ReLU / residual adds and casts in prologues and epilogues;
 * the K|V projections of ALL layers' cross attention hoisted into one GEMM over the raw motion tokens
 * (:43-45 projects the same tokens in every layer); mean-pool over all T rows + classifier (:84,:170).
 * Eval-mode arithmetic (dropout = identity).  Shapes outside the supported set return VMC_E_SHAPE and the
 * caller uses the per-op entry points above.
 *
 * Weights are read from two packs the caller fills once per weight version (vmc_cast_weight / plain copies into
 * the offsets vmc_tfam_pack_offset returns):
 *   wpack  16-bit: per layer self_attn.in_proj_weight [3D,D] | self_attn.out_proj.weight | cross_attn.in_proj_weight[0:D]
 *          | cross_attn.out_proj.weight | ffn.0.weight [ff,D] | ffn.3.weight [D,ff]; then, for l = 0..L-1,
 *          cross_attn.in_proj_weight[D:3D] of layer l ([L*2D, D] in all) | classifier.1.weight | classifier.4.weight
 *   ppack  fp32: per layer the six biases in the same order, norm_self / norm_cross / norm_ffn (weight then bias);
 *          then in_proj_bias[D:3D] per layer | classifier.0 weight, bias | classifier.1.bias | classifier.4.bias
 * vmc_tfam_pack_offset(slot, layer, ...) = element offset of a slot (16-bit elements for W slots, floats for P slots;
 * `layer` is ignored by the global slots except KV_ALL, where it selects that layer's 2D rows); *_END = pack size.
 */
enum {
  VMC_TFAM_W_SELF_IN = 0, VMC_TFAM_W_SELF_OUT, VMC_TFAM_W_CROSS_Q, VMC_TFAM_W_CROSS_OUT, VMC_TFAM_W_FFN0, VMC_TFAM_W_FFN3,
  VMC_TFAM_W_KV_ALL, VMC_TFAM_W_CLS1, VMC_TFAM_W_CLS4, VMC_TFAM_W_END,
  VMC_TFAM_P_SELF_IN_B = 16, VMC_TFAM_P_SELF_OUT_B, VMC_TFAM_P_CROSS_Q_B, VMC_TFAM_P_CROSS_OUT_B, VMC_TFAM_P_FFN0_B,
  VMC_TFAM_P_FFN3_B, VMC_TFAM_P_NORM_SELF, VMC_TFAM_P_NORM_CROSS, VMC_TFAM_P_NORM_FFN, VMC_TFAM_P_KV_ALL_B,
  VMC_TFAM_P_CLS_LN, VMC_TFAM_P_CLS1_B, VMC_TFAM_P_CLS4_B, VMC_TFAM_P_END
};
long long vmc_tfam_pack_offset(int slot, int layer, int D, int ff, int L, int C);
/* Pack-time helper for the three linears that consume a LayerNorm output (self_attn.in_proj of layers >= 1 <- norm_ffn of the
 * previous layer; cross_attn q rows <- norm_self; ffn.0 <- norm_cross, or norm_self when has_cross = 0): the chain feeds them
 * the STANDARDISED rows z = (y - mean) * rstd and expects the affine part folded in,
 *   w16_out[r, k] = W[r, k] * gamma[k],   bias_out[r] = bias[r] + sum_k W[r, k] * beta[k]
 * (LN(y) W^T + b = z (W . gamma)^T + (b + W beta)).  W fp32 [rows, cols] contiguous; every other slot is a plain cast / copy. */
int vmc_tfam_fold_layernorm(const float* W, const float* bias, const float* gamma, const float* beta, void* w16_out,
                            float* bias_out, int rows, int cols, int dtype16, void* stream);
/* Scratch for one forward of B clips (activations of one layer at a time + the hoisted K|V); caller-owned. */
size_t vmc_tfam_workspace_bytes(int B, int T, int Tk, int D, int ff, int L, int C, int has_cross);
/* Host only (no device is touched): 0 when the fused chain takes these shapes -- train = 0: the eval forward below; train = 1: the
 * training chains further down -- else the error code that every entry of that chain returns for them, before any launch.  A caller
 * that has another path for unsupported shapes asks here first. */
int vmc_tfam_supported(int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross, int train);
/* Hoisted cross-attention K|V: ws.kv[B*Tk, L*2D] = motion[B*Tk, D] (fp32) x kv_all^T + bias  (AMO_CLIP.py:43-45, all layers). */
int vmc_tfam_kv_fwd(const float* motion, const void* wpack, const float* ppack, void* workspace, size_t workspace_bytes,
                    int B, int T, int Tk, int D, int H, int ff, int L, int C, int dtype16, void* stream);
/* One AttentionLayer (AMO_CLIP.py:37-51); wpack / ppack as described above, with the LayerNorm-consuming slots folded.  Layer 0 reads the fp32 tokens x_in [B*T, D]; later layers (x_in = NULL)
 * continue from the pre-LayerNorm sum the previous layer left in the workspace.  mask [B,T] / mask_kv [B,Tk]: 1 = real
 * token (the reference's mask_rgb / mask_flow before inversion, :125-126), NULL = all real.  has_cross = 0: self
 * attention + FFN only (rgb-only / flow-only / concatenated-token modes, :136-147,:159-167). */
int vmc_tfam_layer_fwd(const float* x_in, const uint8_t* mask, const uint8_t* mask_kv, const void* wpack, const float* ppack,
                       int layer, void* workspace, size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L,
                       int C, int has_cross, int dtype16, void* stream);
/* logits[B, C] (fp32) = classifier(mean over all T rows of LN_ffn(last layer))  (AMO_CLIP.py:84,:170). */
int vmc_tfam_head_fwd(const void* wpack, const float* ppack, float* logits, void* workspace, size_t workspace_bytes,
                      int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross, int dtype16, void* stream);
/* The same with the mean over the first *pool_len rows of every clip ("POOL LENGTH" below); same launches. */
int vmc_tfam_head_fwd_len(const void* wpack, const float* ppack, float* logits, void* workspace, size_t workspace_bytes,
                          int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross, const int* pool_len, int dtype16,
                          void* stream);
/* kv + L layers + head in one call (AMO_CLIP.forward, :99-171, eval mode). */
int vmc_tfam_forward(const float* x, const float* motion, const uint8_t* mask, const uint8_t* mask_kv, const void* wpack,
                     const float* ppack, float* logits, void* workspace, size_t workspace_bytes, int B, int T, int Tk,
                     int D, int H, int ff, int L, int C, int has_cross, int dtype16, void* stream);
int vmc_tfam_forward_len(const float* x, const float* motion, const uint8_t* mask, const uint8_t* mask_kv, const void* wpack,
                         const float* ppack, float* logits, void* workspace, size_t workspace_bytes, int B, int T, int Tk,
                         int D, int H, int ff, int L, int C, int has_cross, const int* pool_len, int dtype16, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K11-K14 fused, TRAINING — forward + backward of the TFAM block for short clips as two launch chains
 * (TFAM/models/AMO_CLIP.py:37-51,99-171 in train mode under TFAM/train_and_eval.py:66-101: `output = model(...)`,
 * `loss.backward()`).  Same shape set as the eval chain above.
 *
 * Forward: the six launches per layer of the eval chain with the training arithmetic added in place -- LayerNorm with its
 * affine part in the GEMM prologue (unfolded weights), dropout on the attention probabilities inside the attention
 * prologue, the branch dropouts (AMO_CLIP.py:40,45,50 and ffn's own nn.Dropout :27-28) inside the GEMM epilogues -- and the
 * tensors the backward needs written as side outputs (16-bit GEMM operands, pre-norm sums, keep masks, lse).
 * Backward, per layer (8 launches + 1): LayerNorm backward in the PROLOGUE of the dgrad GEMM that consumes the branch
 * gradient (three times), the two dgrad GEMMs with the residual gradient added in the epilogue, vmc_attention_bwd twice,
 * the qkv dgrad, and ONE grouped launch for all seven weight gradients, their bias gradients and the three LayerNorms'
 * parameter gradients.  Gradients are WRITTEN (not accumulated) through the pointers below; NULL = not wanted.
 *
 * Parameters are passed as structs of device pointers (no packing, nothing copied): 16-bit compute copies [N, K] and their
 * transposes [K, N] (what vmc_cast_weights_multi keeps current after every optimiser step), fp32 masters for biases and
 * LayerNorm parameters, fp32 gradient destinations (e.g. views into a flat gradient arena).
 *   w_cross_in = cross_attn.in_proj_weight [3D, D] (q rows 0:D, k|v rows D:3D), wt_cross_in its transpose [D, 3D].
 *
 * Dropout: p_drop (AttentionLayer's dropout: attention probabilities, the three branch dropouts, the FFN's two), p_mlp
 * (classifier.3).  seeds[7*L + 1] host array, each a value or (bit 63) a device address (include "seed arguments"): per layer
 * {self-attn P, self branch, cross-attn P, cross branch, FFN inner, FFN trailing, FFN branch}, then the classifier's.
 * The element index of every mask equals the per-op path's (vmc_dropout on the [M, N] tensor; vmc_attention_fwd's
 * (b, h, q, k)), so both paths draw identical masks from identical seeds.  The backward must be given the same values.
 */
typedef struct vmc_tfam_layer_params {
  const void *w_self_in, *w_self_out, *w_cross_in, *w_cross_out, *w_ffn0, *w_ffn3;          /* 16-bit [N, K] */
  const void *wt_self_in, *wt_self_out, *wt_cross_in, *wt_cross_out, *wt_ffn0, *wt_ffn3;    /* 16-bit [K, N] */
  const float *b_self_in, *b_self_out, *b_cross_in, *b_cross_out, *b_ffn0, *b_ffn3;
  const float *ln_self_g, *ln_self_b, *ln_cross_g, *ln_cross_b, *ln_ffn_g, *ln_ffn_b;
  float *gw_self_in, *gw_self_out, *gw_cross_in, *gw_cross_out, *gw_ffn0, *gw_ffn3;
  float *gb_self_in, *gb_self_out, *gb_cross_in, *gb_cross_out, *gb_ffn0, *gb_ffn3;
  float *g_ln_self_g, *g_ln_self_b, *g_ln_cross_g, *g_ln_cross_b, *g_ln_ffn_g, *g_ln_ffn_b;
} vmc_tfam_layer_params;
typedef struct vmc_tfam_head_params {
  const void *w_cls1, *w_cls4;                   /* 16-bit classifier.1.weight [D/2, D], classifier.4.weight [C, D/2] */
  const float *w32_cls1, *w32_cls4;              /* their fp32 masters (the head's backward is 8..16 rows of work: fp32 FMAs) */
  const float *cls_ln_g, *cls_ln_b, *b_cls1, *b_cls4;
  float *g_cls_ln_g, *g_cls_ln_b, *gw_cls1, *gb_cls1, *gw_cls4, *gb_cls4;
} vmc_tfam_head_params;
/* Saved activations + backward scratch of one step of B clips; caller-owned, must stay untouched between fwd and bwd. */
size_t vmc_tfam_train_workspace_bytes(int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross);
/* Byte offset, inside that workspace, of the fp32 [B*T, D] gradient wrt the last layer's output that vmc_tfam_head_bwd leaves there
 * (the mean-pool's backward; the layer chain only reads it).  -1 for an unsupported shape. */
long long vmc_tfam_train_pool_grad_offset(int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross);
/* AttentionLayer.forward in train mode.  layers = all L structs (layer l > 0 reads layer l-1's norm_ffn);  x_in: the fp32 tokens
 * (layer 0; NULL otherwise); motion: raw fp32 motion tokens [B*Tk, D] (has_cross).  seeds: the 7 seeds of THIS layer. */
int vmc_tfam_layer_train_fwd(const float* x_in, const float* motion, const uint8_t* mask, const uint8_t* mask_kv,
                             const vmc_tfam_layer_params* layers, int layer, void* workspace, size_t workspace_bytes,
                             int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross, float p_drop,
                             const uint64_t* seeds, int dtype16, void* stream);
/* mean-pool + classifier in train mode (AMO_CLIP.py:84,:170), logits fp32 [B, C]. */
int vmc_tfam_head_train_fwd(const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head, float* logits,
                            void* workspace, size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L, int C,
                            int has_cross, float p_mlp, uint64_t seed, int dtype16, void* stream);
int vmc_tfam_head_train_fwd_len(const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head, float* logits,
                                void* workspace, size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L, int C,
                                int has_cross, float p_mlp, uint64_t seed, const int* pool_len, int dtype16, void* stream);
/* Backward of the head: from dlogits fp32 [B, C] to the gradient wrt the last layer's output (left in the workspace) and
 * the classifier's parameter gradients (autograd of AMO_CLIP.py:170-171). */
int vmc_tfam_head_bwd(const float* dlogits, const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head,
                      void* workspace, size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L, int C,
                      int has_cross, float p_mlp, uint64_t seed, int dtype16, void* stream);
/* With a pool length the gradient is dpooled / n on the rows t < n of every clip and 0 on the rows n..T-1; it is the input of the
 * last layer's first dgrad launch, so those rows stay zero down the whole backward chain.  Same *pool_len as the forward. */
int vmc_tfam_head_bwd_len(const float* dlogits, const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head,
                          void* workspace, size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L, int C,
                          int has_cross, float p_mlp, uint64_t seed, const int* pool_len, int dtype16, void* stream);
/* Backward of one AttentionLayer (autograd of AMO_CLIP.py:37-51): consumes the gradient wrt its output from the workspace,
 * leaves the gradient wrt its input there for layer-1 (not computed for layer 0: the tokens need no gradient), writes the
 * layer's parameter gradients.  x_in (layer 0 only) is not read: its 16-bit cast was saved by the forward. */
int vmc_tfam_layer_bwd(const uint8_t* mask, const uint8_t* mask_kv, const vmc_tfam_layer_params* layers, int layer,
                       void* workspace, size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L, int C,
                       int has_cross, float p_drop, const uint64_t* seeds, int dtype16, void* stream);
/* Whole chains: L x layer_train_fwd + head_train_fwd; head_bwd + L x layer_bwd (last layer first). */
int vmc_tfam_train_fwd(const float* x, const float* motion, const uint8_t* mask, const uint8_t* mask_kv,
                       const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head, float* logits, void* workspace,
                       size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross,
                       float p_drop, float p_mlp, const uint64_t* seeds, int dtype16, void* stream);
int vmc_tfam_train_bwd(const float* dlogits, const uint8_t* mask, const uint8_t* mask_kv, const vmc_tfam_layer_params* layers,
                       const vmc_tfam_head_params* head, void* workspace, size_t workspace_bytes, int B, int T, int Tk, int D,
                       int H, int ff, int L, int C, int has_cross, float p_drop, float p_mlp,
                       const uint64_t* seeds, int dtype16, void* stream);
/* The whole chains with a pool length (the `_len` head entries above in place of the plain ones; same launches). */
int vmc_tfam_train_fwd_len(const float* x, const float* motion, const uint8_t* mask, const uint8_t* mask_kv,
                           const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head, float* logits, void* workspace,
                           size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross,
                           float p_drop, float p_mlp, const uint64_t* seeds, const int* pool_len, int dtype16, void* stream);
int vmc_tfam_train_bwd_len(const float* dlogits, const uint8_t* mask, const uint8_t* mask_kv, const vmc_tfam_layer_params* layers,
                           const vmc_tfam_head_params* head, void* workspace, size_t workspace_bytes, int B, int T, int Tk, int D,
                           int H, int ff, int L, int C, int has_cross, float p_drop, float p_mlp,
                           const uint64_t* seeds, const int* pool_len, int dtype16, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K11-K14 fused, TRAINING, feature-concatenation mode — AMO_CLIP with use_cross_attention = false, concat_dim = -1
 * (TFAM/models/AMO_CLIP.py:153-157: x = projection_layer(cat([rgb[:, :-1], motion], -1)), Linear(2 D, D)) on the same chains.
 * The input is the materialised concatenation xcat fp32 [B*T, 2 D]; T is the motion stream's length; there is no cross
 * attention and no motion operand.  What the chains above gain:
 *   forward   one launch in front of layer 0: x = 16bit(xcat) Wp^T + bp (operands rounded to the compute dtype, fp32
 *             accumulation, fp32 output: the per-op path's arithmetic).  Layer 0 reads x where it reads the caller's tokens
 *             otherwise; the 16-bit xcat rows are saved.  28 launches at L = 4.
 *   backward  layer 0 runs the qkv dgrad (dx0 = dy1 + dqkv Wqkv) like every other layer, into the workspace extension, with a
 *             16-bit copy; gw_proj = dx0^T xcat and gb_proj are one more problem of the grouped weight-gradient launch that holds
 *             layer 0's problems.  36 launches at L = 4.  No gradient wrt xcat: the tokens are data.
 * Rows t >= *pool_len of every clip get dx0 = 0 (masked as keys by the caller, not pooled) and add nothing to either gradient.
 * Shapes: vmc_tfam_supported(train) without cross attention, and 4 L + 1 <= 32 weight-gradient problems (L <= 7).
 * The workspace is the training workspace with an extension behind it (vmc_tfam_train_proj_workspace_bytes >
 * vmc_tfam_train_workspace_bytes; every offset of the latter, vmc_tfam_train_pool_grad_offset included, is unchanged), so the
 * per-layer entries above (vmc_tfam_head_bwd_len, vmc_tfam_layer_bwd for layers L-1..1) run on it as they are; layer 0 then takes
 * vmc_tfam_layer0_bwd_proj.  Seeds: as above (the projection has no dropout and draws none).
 */
typedef struct vmc_tfam_proj_params {
  const void *w_proj;                            /* 16-bit projection_layer.weight [D, 2D] */
  const float *b_proj;
  float *gw_proj, *gb_proj;                      /* fp32 [D, 2D], [D]; NULL = not wanted */
} vmc_tfam_proj_params;
/* 0 when the shape takes these chains, else an error code */
int vmc_tfam_proj_supported(int B, int T, int D, int H, int ff, int L, int C);
size_t vmc_tfam_train_proj_workspace_bytes(int B, int T, int D, int H, int ff, int L, int C);
/* Byte offset, inside that workspace, of dx0 fp32 [B*T, D], the gradient wrt the projection's output.  -1: unsupported shape. */
long long vmc_tfam_train_proj_dx0_offset(int B, int T, int D, int H, int ff, int L, int C);
int vmc_tfam_train_fwd_proj(const float* xcat, const vmc_tfam_proj_params* proj, const uint8_t* mask,
                            const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head, float* logits, void* workspace,
                            size_t workspace_bytes, int B, int T, int D, int H, int ff, int L, int C, float p_drop, float p_mlp,
                            const uint64_t* seeds, const int* pool_len, int dtype16, void* stream);
/* The whole backward: head, the dgrad chains of layers L-1..0, one grouped weight-gradient launch per four layers. */
int vmc_tfam_train_bwd_proj(const float* dlogits, const vmc_tfam_proj_params* proj, const uint8_t* mask,
                            const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head, void* workspace,
                            size_t workspace_bytes, int B, int T, int D, int H, int ff, int L, int C, float p_drop, float p_mlp,
                            const uint64_t* seeds, const int* pool_len, int dtype16, void* stream);
/* Layer 0 of the per-layer backward: its dgrad chain with the qkv dgrad, and its own grouped launch with the projection's problem.
 * seeds: the 7 seeds of layer 0. */
int vmc_tfam_layer0_bwd_proj(const vmc_tfam_proj_params* proj, const uint8_t* mask, const vmc_tfam_layer_params* layers,
                             void* workspace, size_t workspace_bytes, int B, int T, int D, int H, int ff, int L, int C, float p_drop,
                             const uint64_t* seeds, int dtype16, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K11-K14 fused, TRAINING, gradients wrt the INPUT TOKENS — for callers whose tokens come out of trainable modules (an adapter in
 * front of TFAM, learned prompt tokens, end-to-end fine-tuning) or who want per-frame saliency.  The forward entries above run
 * unchanged on a LARGER workspace (vmc_tfam_train_input_workspace_bytes: the training workspace, or with proj = 1 the projection
 * mode's, plus an extension behind it; every existing offset is unchanged); the backward entries below do what their namesakes do,
 * bit for bit, and add:
 *   dX      fp32 [B*T, D]     VMC_TFAM_WANT_DX, no projection: layer 0 runs the qkv dgrad dX = dy1 + dqkv Wqkv of the other layers (+1
 *                             launch).  The gradient wrt x of vmc_tfam_train_fwd*.
 *   dMotion fp32 [B*Tk, D]    VMC_TFAM_WANT_DMOTION, cross attention: sum over the layers of dkv_l Wkv_l (Wkv_l = rows D..3D of layer l's
 *                             cross in_proj_weight), one K = 2D launch behind each layer's cross-attention backward (+L launches).
 *                             Layer L-1 writes, the layers below add in the order L-2..0 through the launch's fp32 residual operand:
 *                             one fixed order, so the result repeats bit for bit.  The per-layer entry must therefore be called for
 *                             the layers in that order, as the per-layer backward is anyway.
 *   dXcat   fp32 [B*T, 2D]    projection mode (always wanted there): dx0 Wp, one launch behind layer 0's qkv dgrad (+1 launch).  It
 *                             reads wt_proj, the 16-bit TRANSPOSE [2D, D] of projection_layer.weight, which vmc_tfam_proj_params has
 *                             no field for (its layout is fixed) and which only these entries need.
 * Rows t >= *pool_len of every clip, and motion rows that mask_kv masks, come out as exact zeros.  The parameter gradients are those
 * of the entries above, bit for bit.  16-bit operands, fp32 accumulation, fp32 outputs.
 * Shapes: vmc_tfam_input_grad_supported == 0: those of the chain it extends (vmc_tfam_supported(train) / vmc_tfam_proj_supported).
 * The three gradients live in the extension at vmc_tfam_train_input_grad_offsets; they are valid after the backward call until
 * the workspace is written again.
 */
#define VMC_TFAM_WANT_DX 1
#define VMC_TFAM_WANT_DMOTION 2
/* proj = 1: the feature-concatenation mode, which has no cross attention (has_cross = 1 with it is VMC_E_SHAPE).  0 when the shape is taken. */
int vmc_tfam_input_grad_supported(int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross, int proj);
/* 0: unsupported shape */
size_t vmc_tfam_train_input_workspace_bytes(int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross, int proj);
/* offsets[0..2] = byte offsets of dX, dMotion, dXcat inside that workspace; -1 for a gradient the configuration does not have. */
int vmc_tfam_train_input_grad_offsets(int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross, int proj,
                                      long long* offsets);
/* vmc_tfam_train_bwd_len + the gradients named by `want` (VMC_TFAM_WANT_* bits; 0: exactly vmc_tfam_train_bwd_len). */
int vmc_tfam_train_bwd_inputs_len(const float* dlogits, const uint8_t* mask, const uint8_t* mask_kv,
                                  const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head, void* workspace,
                                  size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L, int C, int has_cross,
                                  float p_drop, float p_mlp, const uint64_t* seeds, const int* pool_len, int want, int dtype16,
                                  void* stream);
/* vmc_tfam_layer_bwd + this layer's part of them: dMotion for every layer, dX for layer 0. */
int vmc_tfam_layer_bwd_inputs(const uint8_t* mask, const uint8_t* mask_kv, const vmc_tfam_layer_params* layers, int layer,
                              void* workspace, size_t workspace_bytes, int B, int T, int Tk, int D, int H, int ff, int L, int C,
                              int has_cross, float p_drop, const uint64_t* seeds, int want, int dtype16, void* stream);
/* vmc_tfam_train_bwd_proj + dXcat */
int vmc_tfam_train_bwd_inputs_proj(const float* dlogits, const vmc_tfam_proj_params* proj, const void* wt_proj, const uint8_t* mask,
                                   const vmc_tfam_layer_params* layers, const vmc_tfam_head_params* head, void* workspace,
                                   size_t workspace_bytes, int B, int T, int D, int H, int ff, int L, int C, float p_drop,
                                   float p_mlp, const uint64_t* seeds, const int* pool_len, int dtype16, void* stream);
/* vmc_tfam_layer0_bwd_proj + dXcat */
int vmc_tfam_layer0_bwd_proj_inputs(const vmc_tfam_proj_params* proj, const void* wt_proj, const uint8_t* mask,
                                    const vmc_tfam_layer_params* layers, void* workspace, size_t workspace_bytes, int B, int T,
                                    int D, int H, int ff, int L, int C, float p_drop, const uint64_t* seeds, int dtype16,
                                    void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K15 — fused Adam / AdamW over one flat fp32 buffer (train.py:66; TFAM/train_and_eval.py:53).
 *   decoupled_wd = 1: p *= 1 - lr*wd first (AdamW); 0: g += wd*p (Adam L2).
 *   grad_scale multiplies g first (clip_grad_norm_ coefficient / DDP averaging).
 */
int vmc_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int decoupled_wd, int step, float grad_scale, void* stream);
/* Device-resident step state for hipGraph-captured training steps (the step count, the bias corrections, the learning rate and
 * the dropout seeds must not be host scalars frozen into the graph -- ADVICE r1).
 *   state  u64 [2 + n_seeds] in device memory: [0] step count t (start at 0), [1] base seed, [2..] this step's dropout seeds
 *   hyper  f32 [4], 16-byte aligned: {lr, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), grad_scale}; the host writes [0] and [3]
 *          (with gradient clipping vmc_grad_clip_dev writes [3], with loss scaling vmc_loss_scale_check does: both below)
 * vmc_train_tick: t += 1, recomputes hyper[1..2] and the n_seeds seeds (splitmix of base seed, t and the index); enqueue it once
 * per step before the forward.  vmc_adam_step_dev = vmc_adam_step reading its four scalars from `hyper`.
 * SEED ARGUMENTS (vmc_dropout, vmc_postnorm_dropout_fwd, vmc_attention_fwd / _bwd, vmc_patch_keep_sample, vmc_drop_path_sample): a value < 2^63 is the
 * seed itself; with bit 63 set the low 63 bits are the ADDRESS of a u64 in device memory holding it (e.g. &state[2 + i]), read at
 * kernel start.
 * POOL LENGTH (the `_len` entries: vmc_mean_pool_len / _bwd_len, vmc_tfam_head_fwd_len, vmc_tfam_forward_len,
 * vmc_tfam_head_train_fwd_len, vmc_tfam_head_bwd_len, vmc_tfam_train_fwd_len / _bwd_len): the same idea for the mean-pool.
 * `pool_len` points to ONE int32 in DEVICE memory, n = the number of leading rows of every clip that enter the mean, read at
 * kernel start -- a captured launch pools over the n of the replay, so one graph serves every batch that was zero-padded (tokens
 * and key masks) from its own length n up to the captured T and gives the unpadded batch's logits and gradients (the reference
 * pools over the batch's padded length, TFAM/models/AMO_CLIP.py:169-170; every other operation is per row or masks the added
 * keys).  The host cannot validate device memory: kernels clamp n into [1, T].  NULL = T, i.e. the entry without the suffix,
 * which is implemented as that call: one kernel body per pool, the same launches either way. */
int vmc_train_tick(void* state, float* hyper, float beta1, float beta2, int n_seeds, void* stream);
int vmc_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                      float eps, float weight_decay, int decoupled_wd, void* stream);
/* The same update launched with at most max_workgroups workgroups of 256 threads: the geometry for an update that runs on a side
 * stream BESIDE other kernels (FusedAdam.enable_backward_overlap: 2 per CU leaves the wave slots the backward's workgroups need). */
int vmc_adam_step_dev_bg(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                         float eps, float weight_decay, int decoupled_wd, int max_workgroups, void* stream);
/* The same update behind a skip flag: `skip` is a DEVICE pointer to one int32 (4-byte aligned).  When *skip != 0 every workgroup
 * returns before its first store (one uniform 4-byte load per workgroup): p, m and v keep their bytes.  skip == NULL is
 * vmc_adam_step_dev_bg, which (like vmc_adam_step_dev) is implemented as this call with NULL.  The flag is the `found_inf` word of
 * a vmc_loss_scale_state (K21). */
int vmc_adam_step_dev_skip(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                           float eps, float weight_decay, int decoupled_wd, int max_workgroups, const int* skip, void* stream);
/* AdamW update AND refresh of the 16-bit compute copies in one pass over the masters (what `optimizer.step()` followed by
 * vmc_cast_weights_multi does in two: TFAM/train_and_eval.py:96 in a captured step).  desc / n_desc / total_tiles: the records of
 * vmc_cast_weights_multi, every `w` pointing into the flat parameter arena p_base; g_base / m_base / v_base are the parallel arenas
 * (element i of a tensor at the same offset in all four).  ranges: DEVICE array of n_ranges records of 16 bytes
 * {uint64 offset; int32 n; int32 block0} for the arena slices that have no compute copy (biases, LayerNorm parameters, ...), record i
 * owning blocks [block0, block0 of i+1) of 1024 elements.  Same arithmetic as vmc_adam_step_dev, bit for bit.  The four bases are
 * 16-byte aligned (VMC_E_ALIGN); a record whose w is not, or whose shape or strides are not multiples of 4, is handled with scalar
 * accesses to the arenas and the copies, as in vmc_cast_weights_multi (not an error). */
int vmc_adam_cast_multi(const void* desc, int n_desc, int total_tiles, const void* ranges, int n_ranges, int total_range_blocks,
                        float* p_base, const float* g_base, float* m_base, float* v_base, const float* hyper, float beta1, float beta2,
                        float eps, float weight_decay, int decoupled_wd, int dtype16, void* stream);
/* vmc_adam_cast_multi behind the skip flag of vmc_adam_step_dev_skip: with *skip != 0 both launches return before their first
 * store, so the masters, m, v AND the 16-bit copies keep their bytes.  NULL = vmc_adam_cast_multi, which is this call with NULL. */
int vmc_adam_cast_multi_skip(const void* desc, int n_desc, int total_tiles, const void* ranges, int n_ranges, int total_range_blocks,
                             float* p_base, const float* g_base, float* m_base, float* v_base, const float* hyper, float beta1,
                             float beta2, float eps, float weight_decay, int decoupled_wd, int dtype16, const int* skip, void* stream);
/* Gradient clipping computed on the device (torch.nn.utils.clip_grad_norm_, train.py:105-106, inside a captured step): the global
 * norm of `grad` (n floats, 16-byte aligned) and from it the factor the Adam kernels read from hyper[3].  Enqueue it after the
 * backward (and, under data parallelism, after the gradient exchange) and before vmc_adam_step_dev / vmc_adam_cast_multi.
 *   clip  f32 [4] in device memory, 16-byte aligned:
 *     [0] base_scale  host-written   what hyper[3] holds without clipping: 1, or 1 / world when `grad` is a sum over ranks
 *     [1] max_norm    host-written   the clipping threshold
 *     [2] norm        device-written ||grad||_2 * |base_scale|: the norm of the AVERAGED gradient
 *     [3] coef        device-written min(1, max_norm / (norm + 1e-6)), torch's coefficient
 *   and hyper[3] = base_scale * coef (device-written: with clipping the host leaves hyper[3] alone and writes clip[0]).
 * Non-finite gradients propagate as in torch (an infinite norm gives coef 0, a NaN norm a NaN coef); nothing is skipped.
 * Two launches, no atomics: workgroup partials (doubles, one per workgroup, in `workspace`: vmc_grad_clip_workspace_bytes(n),
 * 16-byte aligned) are added in a fixed order, so the same gradient gives the same bits on every call and every replay. */
size_t vmc_grad_clip_workspace_bytes(size_t n);
int vmc_grad_clip_dev(const float* grad, size_t n, float* hyper, float* clip, void* workspace, size_t workspace_bytes,
                      void* stream);
/* sum of squares of a flat f32 buffer, accumulated (+=) into out[0] (global grad norm). */
int vmc_sumsq(const float* x, size_t n, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K17 — batch assembly from a device-resident embedding store: HDF5VideoDataset.__getitem__ + collate_fn_pad
 * (TFAM/data/dataset.py:38-51, 76-112) for videos whose rows already sit in device memory.
 *   One launch assembles every stream's padded tokens and mask, the label rows and the max_len values.  The copy is exact (fp32 in,
 *   fp32 out) and EVERY output element is written on every call, padding rows included: a graph replay never sees the bytes of the
 *   previous batch.  16-byte accesses where D % 4 == 0 and `rows` and `out` are 16-byte aligned, 4-byte accesses otherwise (neither
 *   is an error).  `streams` is a HOST array read at enqueue time (as vmc_tfam_layer_params is); everything it points to, `index`,
 *   `labels`, `labels_out` and `status` are device memory.  The call only enqueues: no synchronisation, safe under capture.
 *   max_len: the "POOL LENGTH" value of the assembled batch (above), max over b of min(length, T_out), at least 1, written by one
 *   thread that loops over the B indices (no atomics: the same bits on every replay).
 *   status: sticky, *status |= bits, written by that thread.  Bit 1: an index outside [0, n_videos); bit 2: a clip longer than
 *   T_out was truncated.  The host zeroes it and reads it when it likes (once per epoch, say).
 *   The kernel checks every index BEFORE it forms an address from it (the host cannot validate device memory): an index out of
 *   range gives an empty clip -- zero rows, zero mask, zero label row.  A negative length counts as 0.
 * VMC_E_ARG, before any launch: streams / rows / offset / length / out / mask / index NULL, labels_out NULL or C <= 0 while labels
 * is given, B / D / T_out / n_videos <= 0, n_streams outside 1..2.  VMC_E_SHAPE: B > 65535. */
typedef struct vmc_clip_stream {
  const float* rows;        /* [total_rows, D] fp32, the videos' rows back to back */
  const long long* offset;  /* [n_videos] first row of video i */
  const int* length;        /* [n_videos] rows of video i; 0 is allowed */
  float* out;               /* [B, T_out, D]; rows t >= length are written as zeros */
  uint8_t* mask;            /* [B, T_out]; 1 = real token (arange(T) < length) */
  int* max_len;             /* one int32 in device memory, may be NULL: max over b of min(length, T_out), at least 1 */
  int T_out;
} vmc_clip_stream;
int vmc_gather_clips(const vmc_clip_stream* streams, int n_streams /* 1 or 2 */, const int* index /* device, [B] */, int B,
                     long long n_videos, int D, const float* labels /* [n_videos, C] or NULL */, float* labels_out /* [B, C] */,
                     int C, int* status /* device, one int32, may be NULL */, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K18 — device-resident epoch log: what the TFAM loops keep per step for the epoch's loss and metric (TFAM/train_and_eval.py
 * :86-87,119-122: the logits rows, the label rows, the running loss), appended at a cursor in device memory.  A captured training
 * step then logs itself and the host reads the log once per epoch instead of once per step.
 *   One call, all on the device (enqueue only, no allocation, no synchronisation, safe under capture), with rows = state[0]:
 *   - rows < 0 or rows + B > capacity: status bit 1 is set and NOTHING else is written -- no row, no counter, no loss.
 *   - otherwise the B rows of `values` are copied to values[rows .. rows + B) bit for bit; `targets` receives every label truncated
 *     toward zero (labels.to(torch.int)) and clamped into 0..255 (NaN: 0); status bit 2 is set if a truncated label is not 0 or 1;
 *     squash[rows .. rows + B) = f, f = 1 iff ANY of the B * C values of this call is < 0 or > 1 -- torchmetrics' rule for applying
 *     a sigmoid to an update call, as IEEE comparisons: NaN, -0.0, 0.0 and 1.0 do not set it;
 *   - then loss_sum += *loss (one fp32 add; skipped when loss is NULL), steps += 1, rows += B.
 *   state: [0] rows, [1] steps (accepted calls), [2] status (sticky), [3] reserved.  The host zeroes state and loss_sum to start an
 *   epoch and reads them when it likes.
 *   One launch of one workgroup with 4-byte accesses (the destination offset rows * C is a device value of unknown alignment);
 *   the counters are written by one thread with plain stores, no atomics: the same bits on every call and every replay.
 * VMC_E_ARG, before any launch: log / values / targets or a pointer field of the log NULL, B / C / capacity <= 0. */
typedef struct vmc_metric_log {
  float* values;      /* [capacity, C] fp32: the rows exactly as they were handed in (logits or probabilities) */
  uint8_t* targets;   /* [capacity, C] labels truncated toward zero, as labels.to(torch.int) */
  uint8_t* squash;    /* [capacity] 1: the append call this row came with had a value < 0 or > 1 */
  int* state;         /* [4] int32: rows, steps, status, reserved */
  float* loss_sum;    /* [1] fp32 */
  int capacity, C;
} vmc_metric_log;
int vmc_metric_append(const vmc_metric_log* log, const float* values /* [B, C] */, const float* targets /* [B, C] */,
                      const float* loss /* device, 1 element, or NULL */, int B, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K19 — token concatenation at device-resident lengths: the token-concatenation mode's torch.cat([rgb[:, :-1], motion], 1)
 * (TFAM/models/AMO_CLIP.py:153-156) for streams that were zero-padded beyond their own lengths, with the real rows as a PREFIX of
 * the output, so that one "POOL LENGTH" value (above) serves the concatenated sequence and a captured forward or step replays for
 * every batch of a length bucket.  After the per-stream positional encoding nothing in the layers depends on a row's position: rows
 * 0..n-1 below are exactly the reference's concatenation at the batch's own lengths, the rows behind them are masked as keys, stay
 * out of the pool and receive a zero gradient.
 *   len_rgb / len_motion: ONE int32 each in DEVICE memory, read at kernel start (the "POOL LENGTH" convention): the streams' own
 *   lengths n_rgb / n_motion.  NULL = T_rgb / T_motion.  The host cannot validate device memory, so the kernel clamps:
 *     nr = clamp(*len_rgb, 1, T_rgb);  nm = clamp(*len_motion, 1, T_motion);
 *     keep = min(nr - 1, T_out);  nm = min(nm, T_out - keep);  n = keep + nm  (1 <= n <= T_out).
 *   x    [B, T_out, D] fp32: rgb[b, t] for t < keep, motion[b, t - keep] for keep <= t < n, 0 for n <= t < T_out (exact copies).
 *   mask [B, T_out] u8: the source masks' bytes in the same layout, 1 where a source mask pointer is NULL, 0 on rows n..T_out-1.
 *   pool_len[0] = n, one plain store.
 *   EVERY element of x, mask and pool_len is written on every call (the outputs may be uninitialised; a graph replay never sees the
 *   previous batch), and for any device values nothing outside the buffers is read or written.  With NULL lengths and
 *   T_out = T_rgb - 1 + T_motion the outputs are the reference's torch.cat of tokens and masks.
 *   16-byte accesses where D % 4 == 0 and rgb, motion and x are 16-byte aligned, 4-byte accesses otherwise (neither is an error).
 *   The call only enqueues: no allocation, no synchronisation, safe under capture.
 * VMC_E_ARG, before any launch: rgb / motion / x / mask / pool_len NULL.  VMC_E_SHAPE: B / T_rgb / T_motion / T_out / D <= 0,
 * B > 65535. */
int vmc_concat_tokens_len(const float* rgb, const float* motion, const uint8_t* mask_rgb /* [B, T_rgb] or NULL */,
                          const uint8_t* mask_motion /* [B, T_motion] or NULL */, float* x, uint8_t* mask, int* pool_len, int B,
                          int T_rgb, int T_motion, int T_out, int D, const int* len_rgb, const int* len_motion, void* stream);
/* Its backward: the scatter of dx [B, T_out, D] fp32 to the two streams, lengths read from device memory and clamped as above.
 *   drgb    [B, T_rgb, D]:    dx[b, t] for t < keep, 0 on every other row (the dropped last RGB row and the padding included)
 *   dmotion [B, T_motion, D]: dx[b, keep + t] for t < nm, 0 on the rows behind them
 * Exact copies; every element of both outputs is written on every call, by one pass of plain vector stores (each output row has
 * one source row or none: no atomics).  Rows n..T_out-1 of dx are not read.  Only enqueues; safe under capture.
 * VMC_E_ARG: dx / drgb / dmotion NULL.  VMC_E_SHAPE: as the forward. */
int vmc_concat_tokens_len_bwd(const float* dx, float* drgb, float* dmotion, int B, int T_rgb, int T_motion, int T_out, int D,
                              const int* len_rgb, const int* len_motion, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K20 — gradient accumulation over micro-batches on the flat gradient arena (optim.GradArena.accumulate).  Every backward
 * OVERWRITES its slots of the arena; this pass folds what a backward wrote into an fp32 accumulator, so that k micro-batches with
 * weights B_j / B give the full batch's gradient:
 *   mode 0  acc[i] = weight * g[i]                   first micro-step: acc needs no zeroing (8 B per element)
 *   mode 1  acc[i] = fmaf(weight, g[i], acc[i])      (12 B per element)
 *   mode 2  out[i] = fmaf(weight, g[i], acc[i])      last micro-step; acc is left as it is (12 B per element)
 * g, acc, out: n fp32 each, 16-BYTE ALIGNED (the kernel moves float4; n itself may be any size, the n % 4 tail is done element by
 * element).  out may be g itself (the arena finalises in place); any other overlap between the three buffers is not supported.  out
 * is not touched in modes 0 and 1 (pass g or acc).  The multiply-add is an explicit fmaf -- one rounding, whatever the
 * compiler's contraction setting -- so with a power-of-two weight the result equals sequential fp32 `acc + weight * g` bit for bit.
 * inf and NaN propagate.  One launch, plain vector stores, no atomics: the same bits on every call and every replay.  Only
 * enqueues; safe under capture.
 * Checked in this order, before any launch: g, acc or out NULL, mode outside 0..2 -> VMC_E_ARG; g, acc or out not
 * 16-byte aligned -> VMC_E_ALIGN; n == 0 -> success, nothing launched. */
int vmc_grad_accumulate(const float* g, float* acc, float* out, size_t n, float weight, int mode, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K21 — dynamic loss scaling on the device (torch.amp.GradScaler for float16 training: optim.FusedAdam.enable_loss_scaling).
 * The loss is multiplied by S before the backward so that float16 gradients stay in range; this call, enqueued where
 * vmc_grad_clip_dev would be (after the backward and the gradient exchange, before the `_skip` Adam entries), does what
 * GradScaler.unscale_ + step + update do, without a host read:
 *   found     = any element of `grad` (n floats, 16-byte aligned, any n >= 1) is +-inf or NaN.  Tested per element: a finite value
 *               whose fp32 square overflows is not an overflow.
 *   found_inf = found                                            the skip flag of vmc_adam_step_dev_skip / vmc_adam_cast_multi_skip
 *   with clip (the record of vmc_grad_clip_dev; clip[0] is NOT read, base_scale comes from `ls`):
 *     clip[2] = norm = sqrt(sum g^2) * |base_scale| / S          the norm of the UNSCALED averaged gradient
 *     clip[3] = coef = min(1, clip[1] / (norm + 1e-6))           on overflow: the non-finite norm and the coefficient it gives
 *   hyper[3]  = found ? 0 : base_scale / S * coef                coef = 1 without clip: the Adam kernels unscale as they read
 *   the scale, exactly as torch._amp_update_scale_:
 *     found:  scale *= backoff_factor; growth_tracker = 0; skipped += 1
 *     else:   ++growth_tracker; when it equals growth_interval: scale *= growth_factor unless that is not finite; tracker = 0
 *   found and train_state given (the `state` of vmc_train_tick): state[0] -= 1.  The tick at the start of the step had advanced the
 *     step count; torch does not count a skipped step.  The next tick therefore recomputes the same bias corrections AND THE SAME
 *     DROPOUT SEEDS: the step after a skipped one draws the masks the skipped one drew (on another batch, at another scale).
 * The sum of squares is that of vmc_grad_clip_dev, bit for bit (fp32 squares per thread, doubles across threads, fixed order): with a
 * power-of-two S and no under / overflow, norm, coef and hyper[3] * S equal what vmc_grad_clip_dev gives on the unscaled gradient.
 * Two launches, no atomics; one thread makes the plain stores.  One read of 4 B per parameter; with clipping it REPLACES
 * vmc_grad_clip_dev's pass.  workspace: vmc_loss_scale_workspace_bytes(n), 16-byte aligned.  Only enqueues; safe under capture.
 * VMC_E_ARG: grad / ls / hyper / workspace NULL, n == 0, workspace too small.  VMC_E_ALIGN: grad, ls, hyper, clip or workspace not
 * 16-byte aligned, train_state not 8-byte aligned. */
typedef struct vmc_loss_scale_state {
  float scale;           /* S: host-written at start, device-written afterwards */
  float growth_factor;   /* host: multiplier after growth_interval clean steps */
  float backoff_factor;  /* host: multiplier after an overflow */
  float base_scale;      /* host: what hyper[3] holds without scaling: 1, or 1 / world */
  int growth_interval;   /* host: clean steps before growth */
  int growth_tracker;    /* device: clean steps since the last change */
  int found_inf;         /* device: 0 or 1 for the last checked step; this word is the skip flag */
  int skipped;           /* device: total skipped steps */
} vmc_loss_scale_state;
size_t vmc_loss_scale_workspace_bytes(size_t n);
int vmc_loss_scale_check(const float* grad, size_t n, vmc_loss_scale_state* ls, float* hyper, float* clip, void* train_state,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * K22 — exponential moving average of the trained weights on the flat parameter arena (optim.FusedAdam.enable_ema; DESIGN.md
 * 3.3.6).  One streaming launch after the optimiser's:
 *   ema[i] = fmaf(w, p[i] - ema[i], ema[i])          torch.lerp(ema, p, w): one fp32 subtraction, one fused multiply-add
 *   w = one_minus_decay                               warmup == 0
 *   w = max(one_minus_decay, 9.0f / (float)(10 + t))  warmup == 1: decay_t = min(decay, (1 + t) / (10 + t)) without the cancellation
 * one_minus_decay is 1 - decay ROUNDED BY THE HOST from float64: for decay = 0.9999 an fp32 subtraction on the device would be wrong
 * by about 6e-4 relative.  t is `step` when train_state is NULL; otherwise state[0] of vmc_train_tick (a 64-bit count in device
 * memory, read by the kernel: a captured step replays with the right weight) and `step` is only range-checked.  skip: device
 * pointer to one int32 (the found_inf word of vmc_loss_scale_state) or NULL; when *skip != 0 every workgroup returns before its
 * first store and ema keeps its bytes -- the contract of vmc_adam_step_dev_skip.  ema, p: n fp32 each, 16-BYTE ALIGNED, not
 * overlapping; any n (the n % 4 tail is done element by element).  inf and NaN propagate.  HBM: 12 B per element.  One launch,
 * plain vector stores, no LDS, no atomics: the same bits on every call and every replay.  Only enqueues; safe under capture.
 * Checked in this order, before any launch: ema or p NULL, one_minus_decay outside [0, 1] or NaN, warmup not 0 / 1, step < 0 ->
 * VMC_E_ARG; ema or p not 16-byte aligned, train_state not 8-byte aligned, skip not 4-byte aligned -> VMC_E_ALIGN; n == 0 ->
 * success, nothing launched. */
int vmc_ema_update(float* ema, const float* p, size_t n, float one_minus_decay, int warmup, long long step, const void* train_state,
                   const int* skip, void* stream);

/* vmc_ema_swap: a[i] <-> b[i] for i < n, bit for bit (NaN payloads, -0 and subnormals included): evaluating with the average needs
 * no third arena-sized buffer.  A thread loads both values before it stores either.  HBM: 16 B per element.  Only enqueues.
 * In this order: a or b NULL, a == b, overlapping ranges -> VMC_E_ARG; a or b not 16-byte aligned -> VMC_E_ALIGN; n == 0 ->
 * success, nothing launched. */
int vmc_ema_swap(float* a, float* b, size_t n, void* stream);

/* ---- LoRA adapters on a frozen linear (vimo_clip_amd/lora.py) ----------------------------------------------
 * An adapted linear y = x W^T + s (x A^T) B^T runs the existing GEMM on xcat = [x | ts | 0] and Wcat = [W16 | B16 | 0], both 64
 * columns wider: the adapter term is one more K tile of the fp32 accumulation.  The two launches that are new:
 *
 * vmc_lora_down_concat: for every row m < M
 *     out[m, 0:K]              = x[m, 0:K]                                      bit for bit, when copy_x != 0 (untouched otherwise)
 *     out[m, col0 + j]         = round16(scale * sum_k x[m, k] a16[j, k])       j < r; fp32 MFMA accumulation, one 16-bit rounding
 *     out[m, col0 + r : col0 + 64] = 0
 * x [M, ldx], a16 [r, lda], out [M, ldo] 16-bit; nothing else of out is written.  x is read once: the fragments that feed the MFMAs
 * are the registers stored.  HBM: M K 2 B read, M (K + 64) 2 B written.  The backward calls it with x = dz and a16 = B16^T [r, N].
 * x may be out itself with copy_x == 0 (the first K columns of a concat buffer filled by the caller).
 * Before any launch -- VMC_E_ARG: a NULL pointer.  VMC_E_SHAPE: M < 1, K % 64 != 0, r % 8 != 0 or outside 8..64, col0 < K,
 * col0 % 8 != 0, ldx < K, lda < K, ldo < col0 + 64.  VMC_E_ALIGN: a pointer not 16-byte aligned, a leading dimension % 8 != 0. */
int vmc_lora_down_concat(const void* x, int ldx, const void* a16, int lda, void* out, int ldo, int M, int K, int r, int col0,
                         float scale, int copy_x, int dtype16, void* stream);

/* vmc_lora_wgrad_tn: out[j, c] = sum_m t[m, j] x[m, c], fp32, overwritten; out is [r, C] contiguous, or [C, r] with
 * transpose_out != 0.  t [M, ldt] and x [M, ldx] are 16-bit column windows of wider buffers (what lies beyond r / C columns or M rows
 * is never read).  The tokens are cut into slices whose fp32 slabs are added in slice order: no atomics, the same bits every call.
 * HBM: about M (C + r) 2 B read.  workspace: vmc_lora_wgrad_tn_workspace_bytes(M, r, C) bytes (0 when one slice suffices),
 * 16-byte aligned.  Before any launch -- VMC_E_ARG: t / x / out NULL, workspace NULL or too small.  VMC_E_SHAPE: M < 1, r % 8 != 0
 * or outside 8..64, C % 8 != 0, ldt < r, ldx < C.  VMC_E_ALIGN: a pointer not 16-byte aligned, ldt or ldx % 8 != 0. */
size_t vmc_lora_wgrad_tn_workspace_bytes(int M, int r, int C);
int vmc_lora_wgrad_tn(const void* t, int ldt, const void* x, int ldx, float* out, int M, int r, int C, int transpose_out,
                      void* workspace, size_t workspace_bytes, int dtype16, void* stream);

/* ---- Patch dropout in the student's training stem (vimo_clip_amd/autograd_vit.py) -------------------------------
 * Per frame the class token and Kp of the G = g^2 patch tokens are kept; the tower then runs on Kp + 1 tokens per frame.  Four
 * memory-bound launches, 16-byte accesses where the rows allow, no floating-point atomics: the same bits every call.
 *
 * vmc_patch_keep_sample: keep[f, 0:Kp] = the Kp patches of frame f with the smallest (key, n), key = hash32(seed, f G + n) (the
 * counter hash of vmc_dropout), written in ascending n.  (key, n) is a strict total order, so the set is one definite subset.  seed:
 * see "SEED ARGUMENTS" (a value, or with bit 63 set the device address of one).  keep int32 [F, Kp].  One workgroup per frame.
 * VMC_E_ARG: keep NULL, F < 1.  VMC_E_SHAPE: not 1 <= Kp <= G <= 1024. */
int vmc_patch_keep_sample(uint64_t seed, int F, int G, int Kp, int* keep, void* stream);

/* vmc_gather_rows16: dst[f Kp + j, 0:cols] = src[f G + idx[f, j], 0:cols], bit copies of 16-bit rows (the patch matrix of any of the
 * patch entry points: cols = kpad, 2 kpad or 3 kpad).  ld_src, ld_dst: row strides in elements.  An id outside 0..G-1 is clamped into
 * it.  HBM: F Kp cols 2 B read and written.  VMC_E_ARG: a NULL pointer, F < 1, cols < 1.  VMC_E_SHAPE: not 1 <= Kp <= G, a stride
 * below cols.  Rows that are not 16-byte aligned (cols or a stride % 8 != 0, a pointer) are copied element by element. */
int vmc_gather_rows16(const void* src, int ld_src, const int* idx, int G, void* dst, int ld_dst, int cols, int F, int Kp,
                      void* stream);

/* vmc_assemble_tokens_keep: vmc_assemble_tokens on the kept patches, N' = Kp + 1 tokens per frame:
 *     x[f N', :] = cls + pos[0];   x[f N' + 1 + j, :] = xp[f Kp + j, :] + pos[keep[f, j] + 1, :]
 * one fp32 add and the store rounding of x's type, as vmc_assemble_tokens.  xp 16-bit [F Kp, D]; cls f32 [D]; pos f32 [G + 1, D];
 * keep int32 [F, Kp] (ids outside 0..G-1 are clamped); x [F N', D] f32 or the 16-bit type.  HBM: F Kp D 2 B read, F N' D x B written;
 * the positional table is read through the caches.
 * VMC_E_ARG: a NULL pointer, F < 1, D < 1.  VMC_E_SHAPE: not 1 <= Kp <= G.  VMC_E_DTYPE: x neither f32 nor dtype16. */
int vmc_assemble_tokens_keep(const void* xp, const float* cls, const float* pos, const int* keep, void* x, int F, int G, int Kp,
                             int D, int x_dtype, int dtype16, void* stream);

/* vmc_assemble_tokens_keep_bwd: dx [F N', D] f32 or 16-bit ->
 *     dxp16[f Kp + j, :] = round16(dx[f N' + 1 + j, :])
 *     dpos[0, :] = dcls = sum_f dx[f N', :];   dpos[n + 1, :] = sum over the frames f that kept patch n of dx[f N' + 1 + slot_f(n), :]
 * (exact zeros where no frame kept n; every row of dpos [G + 1, D] is written).  fp32 sums over the frames in ascending order, cut
 * into at most 8 slabs of frames whose partial sums are added in slab order: the order depends on (F, keep) only.
 * workspace: vmc_assemble_tokens_keep_bwd_workspace_bytes(F, G, D) bytes, 16-byte aligned (the inverse of keep, and the slabs).
 * HBM: F N' D dx read twice, F Kp D 2 B written.  VMC_E_ARG: a NULL pointer, F < 1, D < 1, workspace too small.  VMC_E_SHAPE: not
 * 1 <= Kp <= G.  VMC_E_ALIGN: workspace.  VMC_E_DTYPE: dx neither f32 nor dtype16. */
size_t vmc_assemble_tokens_keep_bwd_workspace_bytes(int F, int G, int D);
int vmc_assemble_tokens_keep_bwd(const void* dx, const int* keep, void* dxp16, float* dcls, float* dpos, int F, int G, int Kp, int D,
                                 int dx_dtype, int dtype16, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Stochastic depth that skips dropped frames, in the student's training tower (autograd_vit.py) -----------------
 * Block l keeps K of the F frames of a forward; the block (its GEMMs, attention, backward, saved activations) runs on the K kept frames
 * and the stream of the others passes by:  out[f] = x[f] (f dropped),  out[f] = c x[f] + s Block(x)[f] (f kept),  s = F / K, c = 1 - s.
 * A frame is `row` consecutive elements (N D of the token stream, D of the class rows); all tensors of a call share `dtype` (VMC_F32,
 * VMC_BF16 or VMC_F16).  Five memory-bound launches: 16-byte accesses where row % (16 / element size) == 0 and the pointers are
 * 16-byte aligned, element by element otherwise; fp32 arithmetic and one rounding at the store; no floating-point atomics: the same
 * bits every call.  Frame ids and slots are read from device memory, which the host cannot validate: ids are clamped into 0..F-1.
 * Common to the four data entries, before any launch: a NULL pointer or row == 0 -> VMC_E_ARG; a dtype outside the three ->
 * VMC_E_DTYPE; a pointer that is not a multiple of its element size -> VMC_E_ALIGN.
 *
 * vmc_drop_path_sample: keep[0:K] = the K frames with the smallest (key, f), key = hash32(seed, block F + f) (the counter hash of
 * vmc_dropout and vmc_patch_keep_sample), written in ascending f; slot[f] = the position of f in keep, -1 where f is dropped.  seed:
 * see "SEED ARGUMENTS".  keep int32 [K], slot int32 [F].  One launch of one workgroup (keys in LDS, rank by counting).
 * VMC_E_ARG: keep or slot NULL, block < 0.  VMC_E_SHAPE: not 1 <= K <= F <= 8192. */
int vmc_drop_path_sample(uint64_t seed, int block, int F, int K, int* keep, int* slot, void* stream);

/* vmc_frame_gather: dst[j, :] = src[keep[j], :], bit copies.  src [F, row], dst [K, row].  HBM: K row read and written.
 * VMC_E_SHAPE: not 1 <= K <= F. */
int vmc_frame_gather(const void* src, const int* keep, void* dst, int F, int K, size_t row, int dtype, void* stream);

/* vmc_frame_scatter_add: dx[f, :] = dpass[f, :] + (slot[f] >= 0 ? dsub[slot[f], :] : 0): the backward of a gather that also passes
 * its input on; one fp32 add, rows with slot < 0 are bit copies of dpass.  dpass, dx [F, row]; dsub [K, row] with every slot below K.
 * HBM: (F + K) row read, F row written.  VMC_E_SHAPE: F < 1. */
int vmc_frame_scatter_add(const void* dpass, const void* dsub, const int* slot, void* dx, int F, size_t row, int dtype, void* stream);

/* vmc_drop_path_merge: out[f, :] = slot[f] >= 0 ? c x[f, :] + s y[slot[f], :] : x[f, :] (a bit copy).  Two fp32 products and their
 * sum, each rounded (no contraction), then the store.  x, out [F, row]; y [K, row].  HBM: (F + K) row read, F row written.
 * VMC_E_SHAPE: F < 1. */
int vmc_drop_path_merge(const void* x, const void* y, const int* slot, void* out, int F, size_t row, float c, float s, int dtype,
                        void* stream);

/* vmc_drop_path_merge_bwd: dx[f, :] = slot[f] >= 0 ? c dout[f, :] : dout[f, :] (a bit copy);  dy[j, :] = s dout[keep[j], :]; one launch
 * writes both.  dout, dx [F, row]; dy [K, row].  HBM: (F + K) row read and written.  VMC_E_SHAPE: not 1 <= K <= F. */
int vmc_drop_path_merge_bwd(const void* dout, const int* keep, const int* slot, void* dx, void* dy, int F, int K, size_t row, float c,
                            float s, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VMC_H */
