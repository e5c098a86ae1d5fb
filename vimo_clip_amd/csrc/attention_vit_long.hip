// CLIP ViT self-attention past the in-LDS kernel's 288 tokens (gfx950): head_dim 64, no mask, bf16 / f16.
// vmc_attention_vit_fwd / vmc_attention_vit_cls_fwd (attention.hip, attn_route.h) dispatch here for N > 288 (ViT-L/14@336px: N = 577).
//
//   full    : one workgroup = 4 waves = one (frame, head, block of 128 query rows); a wave owns two 16-row query tiles whose Q
//             fragments stay in registers.  K / V move in 64-key tiles through two LDS buffers, staged through registers: the next
//             tile's global loads are issued before this tile's MFMAs and written to LDS behind them, one barrier per tile.  K uses the
//             XOR-swizzled image of attn_vit_kernel (lds_off_x), V the ds_read_b64_tr_b16 image (lds_off_v).  Every K and V fragment
//             read from LDS feeds both query tiles.  S^T = K Q^T puts a query's scores in 4 lanes; the online softmax runs on exp2 of
//             pre-scaled scores and the P values, packed to 16 bits, are the B operand of O^T += V^T P^T.  Row sums come from the
//             rounded P (1^T P^T on the MFMA), as in attn_vit_kernel.
//   class   : the NQ = 1 call of the last encoder block (a decode-shaped, K / V bandwidth bound call): one wave per (frame, head), each
//             with its own double-buffered K / V tiles, the keys in the same tile order through the same tile step as the full kernel,
//             so the class row equals row 0 of the full call bit for bit.
//
// N = 577 is instantiated at compile time: only the tile that straddles N compares keys, and its 16-key blocks past N skip their MFMAs.
// Any other N > 288 takes the runtime-N instance (no upper limit).  Keys past N are staged as zero rows, so no stale LDS reaches an MFMA.
// Built with -fno-honor-nans like attention.hip: scores are finite or -inf.
#include "common.h"
#include "attn_route.h"

namespace {

constexpr int KT = ATT_VL_KT;                 // keys per K / V tile
constexpr int TILE_BYTES = KT * 128;          // one 64-key x 64-column 16-bit image
constexpr int BUF_BYTES = 2 * TILE_BYTES;     // K | V
constexpr int NW = ATT_VL_NW;                 // waves per workgroup (both kernels)
constexpr int QROWS = ATT_VL_QROWS;           // query rows per workgroup of the full kernel
static_assert(NW * 2 * BUF_BYTES == ATT_VL_CLS_LDS, "the class-query kernel's per-wave K / V buffers");
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float vmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// One 64-key tile for QT 16-row query tiles of a wave.  NV = 64: a full tile; 0 < NV < 64: the straddling tile of a compile-time N
// with NV live keys (16-key blocks past them skip their MFMAs, 32-key steps past them skip P V); NV = 0: the straddling tile of a
// runtime N with nv live keys.  The arithmetic of one query row does not depend on QT or on the other rows.
template <typename T, int QT, int NV>
__device__ __forceinline__ void vit_tile(const char* kl, const char* vl, int koff0, int koff1, const int (&voff)[4], const uint4 (&qf)[QT][2],
                                         int nv, int q, float c2, float (&m)[QT], f32x4 (&o)[QT][4], f32x4 (&osum)[QT]) {
  constexpr int NB = NV > 0 ? (NV + 15) / 16 : 4;       // 16-key blocks that hold a live key
  constexpr int NKS = (NB + 1) / 2;                     // 32-key steps
  f32x4 s[QT][4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    if (nt >= NB) {
#pragma unroll
      for (int a = 0; a < QT; ++a) s[a][nt] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      continue;
    }
    const uint4 k0 = *(const uint4*)(kl + koff0 + nt * 2048), k1 = *(const uint4*)(kl + koff1 + nt * 2048);
#pragma unroll
    for (int a = 0; a < QT; ++a) {
      s[a][nt] = T::mfma16(k0, qf[a][0], (f32x4){0.f, 0.f, 0.f, 0.f});
      s[a][nt] = T::mfma16(k1, qf[a][1], s[a][nt]);
    }
  }
  if constexpr (NV != KT) {
    const int lim = NV > 0 ? NV : nv;
#pragma unroll
    for (int nt = 0; nt < NB; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (16 * nt + 4 * q + j >= lim) {
#pragma unroll
          for (int a = 0; a < QT; ++a) s[a][nt][j] = -INFINITY;
        }
  }
  uint4 pf[QT][NKS];
#pragma unroll
  for (int a = 0; a < QT; ++a) {
    float mx = vmax3(s[a][0][0], s[a][0][1], vmax3(s[a][0][2], s[a][0][3], -INFINITY));
#pragma unroll
    for (int nt = 1; nt < NB; ++nt) mx = vmax3(vmax3(mx, s[a][nt][0], s[a][nt][1]), s[a][nt][2], s[a][nt][3]);
    mx = vmax3(mx, __shfl_xor(mx, 16, 64), -INFINITY);
    mx = vmax3(mx, __shfl_xor(mx, 32, 64), -INFINITY);
    // every tile holds a live key, so mnew is finite; before the first tile m = -inf and alpha = exp2(-inf) = 0
    const float mnew = vmax3(m[a], mx, -INFINITY);
    const float alpha = __builtin_amdgcn_exp2f((m[a] - mnew) * c2);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[a][dt] *= alpha;
    osum[a] *= alpha;
    m[a] = mnew;
    const float mc = mnew * c2;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const f32x4 x = s[a][2 * ks], y = s[a][2 * ks + 1];
      pf[a][ks].x = pack2<T>(__builtin_amdgcn_exp2f(__builtin_fmaf(x[0], c2, -mc)), __builtin_amdgcn_exp2f(__builtin_fmaf(x[1], c2, -mc)));
      pf[a][ks].y = pack2<T>(__builtin_amdgcn_exp2f(__builtin_fmaf(x[2], c2, -mc)), __builtin_amdgcn_exp2f(__builtin_fmaf(x[3], c2, -mc)));
      pf[a][ks].z = pack2<T>(__builtin_amdgcn_exp2f(__builtin_fmaf(y[0], c2, -mc)), __builtin_amdgcn_exp2f(__builtin_fmaf(y[1], c2, -mc)));
      pf[a][ks].w = pack2<T>(__builtin_amdgcn_exp2f(__builtin_fmaf(y[2], c2, -mc)), __builtin_amdgcn_exp2f(__builtin_fmaf(y[3], c2, -mc)));
    }
  }
  const uint4 ones = make_uint4(T::ONE_PAIR, T::ONE_PAIR, T::ONE_PAIR, T::ONE_PAIR);
  // V^T fragments (tile_index.h attn_pv_key): this lane supplies key 32 ks + 4 q + (r >> 2) (+16) of each 4-key x 16-column block
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    uint4 vf[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const uint2 x0 = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((VMC_LDS s16x4*)(vl + voff[dt] + ks * 4096)));
      const uint2 x1 = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((VMC_LDS s16x4*)(vl + voff[dt] + ks * 4096 + 2048)));
      vf[dt] = make_uint4(x0.x, x0.y, x1.x, x1.y);
    }
#pragma unroll
    for (int a = 0; a < QT; ++a) {
      osum[a] = T::mfma16(ones, pf[a][ks], osum[a]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[a][dt] = T::mfma16(vf[dt], pf[a][ks], o[a][dt]);
    }
  }
}

// Per-lane LDS offsets of the K fragments (keys r, chunks q and 4 + q of every 16-key block) and the V^T fragments.
struct LaneOffsets {
  int koff0, koff1, voff[4];
  __device__ __forceinline__ explicit LaneOffsets(int r, int q) {
    koff0 = lds_off_x(r, q);
    koff1 = lds_off_x(r, 4 + q);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) voff[dt] = lds_off_v(4 * q + (r >> 2), 2 * dt + ((r & 3) >> 1)) + (r & 1) * 8;
  }
};

// The key loop shared by both kernels: tile kt of this head's K / V is in buffer kt & 1 (K | V images, BUF_BYTES apart); stage(kt)
// issues tile kt's global loads into registers, put(buf) writes them.  NC > 0: full tiles, then the straddling one; runtime N: one body
// that compares keys on every tile (a second, compare-free copy of the body made hipcc spill).
template <typename T, int QT, int NC, typename Stage, typename Put>
__device__ __forceinline__ void key_loop(char* bufs, int N, const LaneOffsets& lo, const uint4 (&qf)[QT][2], int q, float c2, bool compute,
                                         float (&m)[QT], f32x4 (&o)[QT][4], f32x4 (&osum)[QT], Stage stage, Put put) {
  const int nkt = (N + KT - 1) / KT, nfull = N / KT;
  for (int kt = 0; kt < nkt; ++kt) {
    const char* kl = bufs + (kt & 1) * BUF_BYTES;
    const char* vl = kl + TILE_BYTES;
    if (kt + 1 < nkt) stage(kt + 1);                     // next tile's loads in flight under this tile's MFMAs
    if (compute) {
      if constexpr (NC > 0) {
        if (kt < nfull) vit_tile<T, QT, KT>(kl, vl, lo.koff0, lo.koff1, lo.voff, qf, KT, q, c2, m, o, osum);
        else if constexpr (NC % KT != 0) vit_tile<T, QT, NC % KT>(kl, vl, lo.koff0, lo.koff1, lo.voff, qf, NC % KT, q, c2, m, o, osum);
      } else {
        vit_tile<T, QT, 0>(kl, vl, lo.koff0, lo.koff1, lo.voff, qf, min(KT, N - kt * KT), q, c2, m, o, osum);
      }
    }
    if (kt + 1 < nkt) put(bufs + ((kt + 1) & 1) * BUF_BYTES);   // that buffer was last read in tile kt - 1, before the barrier that ended it
    __syncthreads();
  }
}

// 64 rows of a head (row0 ..) as 16-byte chunks: the NTHR threads of `t` take chunks t, t + NTHR, ..; rows past N are zero.
template <int NTHR>
struct TileStage {
  static constexpr int IT = KT * 8 / NTHR;
  uint4 k[IT], v[IT];
  __device__ __forceinline__ void load(const uint16_t* kb, const uint16_t* vb, size_t ld, int row0, int N, int t) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int idx = t + NTHR * i, row = idx >> 3, c = idx & 7;
      k[i] = v[i] = make_uint4(0, 0, 0, 0);
      if (row0 + row < N) {
        k[i] = *(const uint4*)(kb + (size_t)(row0 + row) * ld + c * 8);
        v[i] = *(const uint4*)(vb + (size_t)(row0 + row) * ld + c * 8);
      }
    }
  }
  __device__ __forceinline__ void store(char* buf, int t) const {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int idx = t + NTHR * i, row = idx >> 3, c = idx & 7;
      *(uint4*)(buf + lds_off_x(row, c)) = k[i];
      *(uint4*)(buf + TILE_BYTES + lds_off_v(row, c)) = v[i];
    }
  }
};

template <typename T>
__device__ __forceinline__ void store_rows(uint16_t* orow, const f32x4 (&o)[4], float inv) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *(uint2*)(orow + 16 * dt) = make_uint2(pack2<T>(o[dt][0] * inv, o[dt][1] * inv), pack2<T>(o[dt][2] * inv, o[dt][3] * inv));
}

// ---- full call: NQ = N query rows per frame ----
template <typename T, int NC>
__global__ void __launch_bounds__(64 * NW, 3) attn_vit_long_kernel(const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
                                                                const uint16_t* __restrict__ vp, uint16_t* __restrict__ out,
                                                                float* __restrict__ lse, int Nrt, int H, size_t ldq, size_t ldkv, float scale) {
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF_BYTES];     // K0 V0 | K1 V1
  const int N = NC > 0 ? NC : Nrt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int nqb = (N + QROWS - 1) / QROWS;
  // blocks of one (frame, head) are consecutive after the remap, so they run on one XCD and share its L2 copy of K / V
  const int blk = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = blk / nqb, f = bh / H, h = bh % H, D = H * 64;
  const int row0 = (blk % nqb) * QROWS + wave * 32;                      // first query row of this wave
  const uint16_t* kb = kp + (size_t)f * N * ldkv + h * 64;
  const uint16_t* vb = vp + (size_t)f * N * ldkv + h * 64;

  uint4 qf[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const uint16_t* qr = qp + ((size_t)f * N + min(row0 + 16 * a + r, N - 1)) * ldq + h * 64;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[a][kk] = *(const uint4*)(qr + (4 * kk + q) * 8);
  }
  TileStage<64 * NW> st;
  st.load(kb, vb, ldkv, 0, N, tid);
  st.store(smem, tid);
  __syncthreads();

  const LaneOffsets lo(r, q);
  float m[2] = {-INFINITY, -INFINITY};
  f32x4 o[2][4], osum[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    osum[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[a][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  key_loop<T, 2, NC>(smem, N, lo, qf, q, scale * LOG2E, row0 < N, m, o, osum,
                     [&](int kt) { st.load(kb, vb, ldkv, kt * KT, N, tid); }, [&](char* buf) { st.store(buf, tid); });
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int qrow = row0 + 16 * a + r;
    if (qrow < N) {
      const float sum = osum[a][0];    // every accumulator row holds the row sum of query r (16-bit rounded P, as P V uses)
      store_rows<T>(out + ((size_t)f * N + qrow) * D + h * 64 + 4 * q, o[a], 1.0f / sum);
      if (lse != nullptr && q == 0) lse[((size_t)f * H + h) * N + qrow] = m[a] * scale + __logf(sum);
    }
  }
}

// ---- class-query call: one wave per (frame, head), NQ = 1 ----
template <typename T, int NC>
__global__ void __launch_bounds__(64 * NW) attn_vit_long_cls_kernel(const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
                                                                    const uint16_t* __restrict__ vp, uint16_t* __restrict__ out, int Nrt,
                                                                    int H, int n_bh, size_t ldq, size_t ldkv, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];          // per wave: K0 V0 | K1 V1
  const int N = NC > 0 ? NC : Nrt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int bh = blockIdx.x * NW + wave;
  const int bhc = min(bh, n_bh - 1);        // waves past the last (frame, head) repeat it and store nothing: the barriers stay matched
  const int f = bhc / H, h = bhc % H, D = H * 64;
  char* const bufs = smem + wave * 2 * BUF_BYTES;
  const uint16_t* kb = kp + (size_t)f * N * ldkv + h * 64;
  const uint16_t* vb = vp + (size_t)f * N * ldkv + h * 64;

  uint4 qf[1][2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) qf[0][kk] = *(const uint4*)(qp + (size_t)f * ldq + h * 64 + (4 * kk + q) * 8);   // every lane: row 0
  TileStage<64> st;
  st.load(kb, vb, ldkv, 0, N, lane);
  st.store(bufs, lane);
  __syncthreads();

  const LaneOffsets lo(r, q);
  float m[1] = {-INFINITY};
  f32x4 o[1][4], osum[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[0][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  key_loop<T, 1, NC>(bufs, N, lo, qf, q, scale * LOG2E, true, m, o, osum,
                     [&](int kt) { st.load(kb, vb, ldkv, kt * KT, N, lane); }, [&](char* buf) { st.store(buf, lane); });
  if (bh < n_bh && r == 0) store_rows<T>(out + (size_t)f * D + h * 64 + 4 * q, o[0], 1.0f / osum[0][0]);
}

template <typename T, int NC>
int launch(const AttnPlan& pl, const AttnVitProblem& p, hipStream_t s) {
  const uint16_t *q = (const uint16_t*)p.q, *k = (const uint16_t*)p.k, *v = (const uint16_t*)p.v;
  if (pl.kernel == ATTN_VIT_LONG_CLS) {
    auto kern = attn_vit_long_cls_kernel<T, NC>;
    static bool lds_set = false;
    if (int rc = set_max_lds(lds_set, pl.lds, kern)) return rc;
    hipLaunchKernelGGL(kern, dim3(pl.grid[0]), dim3(pl.block), pl.lds, s, q, k, v, (uint16_t*)p.out, p.N, p.H, p.F * p.H, p.ldq, p.ldkv,
                       0.125f);
  } else {
    hipLaunchKernelGGL((attn_vit_long_kernel<T, NC>), dim3(pl.grid[0]), dim3(pl.block), 0, s, q, k, v, (uint16_t*)p.out, p.lse, p.N, p.H,
                       p.ldq, p.ldkv, 0.125f);
  }
  VMC_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// The executor of attn_route.h's ATTN_VIT_LONG / ATTN_VIT_LONG_CLS plans (declared in common.h).
int attn_vit_long_fwd(const AttnPlan& pl, const AttnVitProblem& p, hipStream_t s) {
  if (p.dtype16 == VMC_BF16) return pl.nc == ATT_VL_NC ? launch<BF16, ATT_VL_NC>(pl, p, s) : launch<BF16, 0>(pl, p, s);
  return pl.nc == ATT_VL_NC ? launch<F16, ATT_VL_NC>(pl, p, s) : launch<F16, 0>(pl, p, s);
}
