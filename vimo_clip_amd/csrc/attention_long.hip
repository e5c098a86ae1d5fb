// Tiled ("flash") masked attention on MFMA for sequences of any length (gfx950): head_dim 64 / 96, bf16 / f16.
// vmc_attention_fwd / vmc_attention_bwd (attention.hip) dispatch here every shape their short-sequence kernels do not take:
// the forward beyond 64 keys, the backward once Q, K, V and dO of a head no longer fit in LDS (conditions: attn_route.h).
//
//   forward : one workgroup = 4 waves = one (batch, head, block of 64 query rows); a wave owns 16 query rows.  K / V tiles of
//             64 keys stream through two LDS buffers (the next tile's global loads are issued before this tile's MFMAs and
//             written behind them: one barrier per tile).  S^T = K Q^T puts a query's scores in 4 lanes (lane r = query,
//             keys 4q + j of each 16-key block), the online softmax keeps the running max / sum per lane, and the exponentiated
//             scores, packed to 16 bits, are directly the B operand of O^T += V^T P^T (V^T by ds_read_b64_tr_b16).
//   backward: delta = rowsum(dO o O) into the workspace, then two passes with no atomics (deterministic):
//             pass 1, one workgroup per (b, h, 64 keys): loops over 64-row query tiles of Q | dO in LDS, recomputes P from
//             Q K^T and the lse, accumulates dV^T += dO^T P and dK^T += Q^T dS in registers (key on the lane);
//             pass 2, one workgroup per (b, h, 64 queries): loops over 64-key tiles of K | V in LDS, dQ^T += K^T dS^T.
//
// Key-padding mask: any pattern.  A tile whose 64 keys are all masked is skipped (a ballot over the tile's keys: the same value in
// every wave of the workgroup, so the skip is workgroup-uniform and the barriers stay matched); its dK / dV rows are written as
// zeros.  Padded QUERY rows are computed like any other (the reference mean-pools over them).  A row whose keys are all masked
// yields NaN in out and lse, written as a constant: this file is built like attention.hip with -fno-honor-nans, where NaN
// arithmetic may be folded away.
#include "common.h"
#include "attn_route.h"

namespace {

constexpr int LT = ATT_LONG_LT;      // rows of every tile (queries per workgroup, keys per K / V tile)
constexpr int NTH = ATT_LONG_NTH;    // 4 waves
constexpr float LOG2E = 1.4426950408889634f;

template <typename T>
__device__ __forceinline__ uint32_t nan_pair() { return T::id == VMC_BF16 ? 0x7FC07FC0u : 0x7E007E00u; }

// A 64-row x DH tile of 16-bit elements in LDS, rows padded by 16 B (as attn_small_kernel).  The 256 threads move it in
// DH / 32 16-byte chunks each; rows past `nrows` are zero (the MFMAs then see 0 instead of stale LDS).
template <int DH>
struct TileIO {
  static constexpr int CH = DH / 8, RS = DH * 2 + 16, IT = LT * CH / NTH, BYTES = LT * RS;
  static_assert(LT * CH % NTH == 0, "whole chunks per thread");
  __device__ static __forceinline__ void load(uint4 (&reg)[IT], const uint16_t* base, size_t ld, int row0, int nrows, int tid) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int idx = tid + NTH * i, row = idx / CH, c = idx % CH;
      reg[i] = make_uint4(0, 0, 0, 0);
      if (row0 + row < nrows) reg[i] = *(const uint4*)(base + (size_t)(row0 + row) * ld + c * 8);
    }
  }
  __device__ static __forceinline__ void store(char* lds, const uint4 (&reg)[IT], int tid) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int idx = tid + NTH * i, row = idx / CH, c = idx % CH;
      *(uint4*)(lds + row * RS + c * 16) = reg[i];
    }
  }
};

// Bit i: key key0 + i exists and is not masked.  Every wave computes the same value.
__device__ __forceinline__ uint64_t live_keys(const uint8_t* mb, int key0, int Tk, int lane) {
  const int key = key0 + lane;
  return __ballot(key < Tk && (mb == nullptr || mb[key] != 0));
}

// 16-bit transposed 4-row x 16-column block pair (rows row0, row0 + 16) as one MFMA operand: this lane supplies row
// row0 + 4 g + (r >> 2), columns col0 + 4 (r & 3) ..  (ds_read_b64_tr_b16; EXEC must be full)
__device__ __forceinline__ uint4 tr_pair(const char* lds, int off, int RS) {
  const uint2 x0 = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((VMC_LDS s16x4*)(lds + off)));
  const uint2 x1 = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((VMC_LDS s16x4*)(lds + off + 16 * RS)));
  return make_uint4(x0.x, x0.y, x1.x, x1.y);
}

// ==================================================================================================
// Forward
// ==================================================================================================
template <typename T, int DH>
__global__ void __launch_bounds__(NTH) attn_long_fwd_kernel(const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
                                                            const uint16_t* __restrict__ vp, const uint8_t* __restrict__ mask,
                                                            uint16_t* __restrict__ op, float* __restrict__ lse, int H, int Tq, int Tk,
                                                            int ldq, int ldk, int ldv, int ldo, float scale, float drop_p,
                                                            uint64_t seed_arg) {
  using IO = TileIO<DH>;
  constexpr int KK = DH / 32, DT = DH / 16, RS = IO::RS;
  __shared__ __attribute__((aligned(16))) char smem[4 * IO::BYTES];     // K0 V0 | K1 V1
  const uint64_t seed = drop_p > 0.f ? resolve_seed(seed_arg) : 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int nqb = (Tq + LT - 1) / LT;
  const int bh = blockIdx.x / nqb, b = bh / H, h = bh % H;
  const int qrow = (blockIdx.x % nqb) * LT + wave * 16 + r;
  const uint16_t* kb = kp + (size_t)b * Tk * ldk + h * DH;
  const uint16_t* vb = vp + (size_t)b * Tk * ldv + h * DH;
  const uint8_t* mb = mask != nullptr ? mask + (size_t)b * Tk : nullptr;

  uint4 qf[KK];
  {
    const uint16_t* qr = qp + ((size_t)b * Tq + min(qrow, Tq - 1)) * ldq + h * DH;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[kk] = *(const uint4*)(qr + (4 * kk + q) * 8);
  }
  uint4 kr[IO::IT], vr[IO::IT];
  uint64_t live = live_keys(mb, 0, Tk, lane);
  if (live) {
    IO::load(kr, kb, ldk, 0, Tk, tid);
    IO::load(vr, vb, ldv, 0, Tk, tid);
    IO::store(smem, kr, tid);
    IO::store(smem + IO::BYTES, vr, tid);
  }
  __syncthreads();

  const float c2 = scale * LOG2E;
  const size_t drow = (((size_t)b * H + h) * Tq + min(qrow, Tq - 1)) * (size_t)Tk;    // dropout index of (b, h, qrow, key 0)
  float m = -INFINITY, lsum = 0.f;       // running max (raw score) and this lane's share of the running sum
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nkt = (Tk + LT - 1) / LT;
  for (int kt = 0; kt < nkt; ++kt) {
    const char* kl = smem + (kt & 1) * 2 * IO::BYTES;
    const char* vl = kl + IO::BYTES;
    uint64_t live_next = 0;
    if (kt + 1 < nkt) {                  // next tile's loads in flight under this tile's MFMAs
      live_next = live_keys(mb, (kt + 1) * LT, Tk, lane);
      if (live_next) {
        IO::load(kr, kb, ldk, (kt + 1) * LT, Tk, tid);
        IO::load(vr, vb, ldv, (kt + 1) * LT, Tk, tid);
      }
    }
    if (live) {
      f32x4 s[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        s[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) s[nt] = T::mfma16(*(const uint4*)(kl + (16 * nt + r) * RS + (4 * kk + q) * 16), qf[kk], s[nt]);
      }
      if (live != ~0ull) {               // partly masked (or the last, partial) tile
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (!((live >> (16 * nt + 4 * q + j)) & 1)) s[nt][j] = -INFINITY;
      }
      float mx = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) mx = fmaxf(fmaxf(mx, fmaxf(s[nt][0], s[nt][1])), fmaxf(s[nt][2], s[nt][3]));
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // the tile holds a live key, so mx and mnew are finite; before the first live tile m = -inf and alpha = exp2(-inf) = 0
      const float mnew = fmaxf(m, mx);
      const float alpha = __builtin_amdgcn_exp2f((m - mnew) * c2);
      m = mnew;
      lsum *= alpha;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
      const float mc = mnew * c2;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        float pe[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pe[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[2 * ks][j], c2, -mc));
          pe[4 + j] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[2 * ks + 1][j], c2, -mc));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) lsum += pe[j];      // the softmax denominator does not see the dropout
        if (drop_p > 0.f) {
          const size_t base = drow + kt * LT + 32 * ks + 4 * q;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            pe[j] *= dropout_factor(drop_p, seed, base + j);
            pe[4 + j] *= dropout_factor(drop_p, seed, base + 16 + j);
          }
        }
        const uint4 pf = make_uint4(pack2<T>(pe[0], pe[1]), pack2<T>(pe[2], pe[3]), pack2<T>(pe[4], pe[5]), pack2<T>(pe[6], pe[7]));
        // V^T blocks: keys 32 ks + 4 q + (r >> 2) (+16), columns 16 dt + 4 (r & 3): k-slots 8 q .. 8 q + 7 of pf
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          o[dt] = T::mfma16(tr_pair(vl, (32 * ks + 4 * q + (r >> 2)) * RS + (16 * dt + 4 * (r & 3)) * 2, RS), pf, o[dt]);
      }
    }
    if (live_next) {
      char* kn = smem + ((kt + 1) & 1) * 2 * IO::BYTES;   // last read in tile kt - 1, before the barrier that ended it
      IO::store(kn, kr, tid);
      IO::store(kn + IO::BYTES, vr, tid);
    }
    __syncthreads();
    live = live_next;
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  if (qrow < Tq) {
    uint16_t* orow = op + ((size_t)b * Tq + qrow) * ldo + h * DH + 4 * q;
    const bool dead = m == -INFINITY;   // no live key at all (the batch's mask is all zero)
    const float inv = dead ? 0.f : 1.0f / lsum;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      uint2 w = make_uint2(pack2<T>(o[dt][0] * inv, o[dt][1] * inv), pack2<T>(o[dt][2] * inv, o[dt][3] * inv));
      if (dead) w = make_uint2(nan_pair<T>(), nan_pair<T>());
      *(uint2*)(orow + 16 * dt) = w;
    }
    if (lse != nullptr && q == 0)      // stored as bits: a float select may carry the no-NaN flag
      ((uint32_t*)lse)[((size_t)b * H + h) * Tq + qrow] = dead ? 0x7FC00000u : __float_as_uint(m * scale + __logf(lsum));
  }
}

// ==================================================================================================
// Backward
// ==================================================================================================
// delta[b, h, t] = sum_d dO[b, t, h, d] * O[b, t, h, d]: four lanes per (b, h, t), t fastest.
template <typename T, int DH>
__global__ void __launch_bounds__(256) attn_long_delta_kernel(const uint16_t* __restrict__ op, const uint16_t* __restrict__ dop,
                                                              float* __restrict__ delta, int H, int Tq, int ldo, size_t items) {
  constexpr int CH = DH / 8;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t item = gid >> 2;
  const int part = (int)(gid & 3);
  float dl = 0.f;
  if (item < items) {
    const int t = (int)(item % Tq);
    const size_t bh = item / Tq;
    const int h = (int)(bh % H), b = (int)(bh / H);
    const size_t row = ((size_t)b * Tq + t) * ldo + h * DH;
#pragma unroll
    for (int c = part; c < CH; c += 4) {
      const uint4 ow = *(const uint4*)(op + row + c * 8), dw = *(const uint4*)(dop + row + c * 8);
      const uint32_t oa[4] = {ow.x, ow.y, ow.z, ow.w}, da[4] = {dw.x, dw.y, dw.z, dw.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float o0, o1, d0, d1;
        unpack2<T>(oa[j], o0, o1);
        unpack2<T>(da[j], d0, d1);
        dl += o0 * d0 + o1 * d1;
      }
    }
  }
  dl += __shfl_xor(dl, 1, 64);
  dl += __shfl_xor(dl, 2, 64);
  if (item < items && part == 0) delta[item] = dl;
}

// Pass 1: dK, dV of 64 keys (a wave owns 16: lane r = key, registers = queries 4 g + j of each 16-row block).
template <typename T, int DH>
__global__ void __launch_bounds__(NTH) attn_long_bwd_kv_kernel(const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
                                                               const uint16_t* __restrict__ vp, const uint8_t* __restrict__ mask,
                                                               const uint16_t* __restrict__ dop, const float* __restrict__ lse,
                                                               const float* __restrict__ delta, uint16_t* __restrict__ dkp,
                                                               uint16_t* __restrict__ dvp, int H, int Tq, int Tk, int ldq, int ldk,
                                                               int ldv, int ldo, int lddk, int lddv, float scale, float drop_p,
                                                               uint64_t seed_arg) {
  using IO = TileIO<DH>;
  constexpr int KK = DH / 32, DT = DH / 16, RS = IO::RS;
  constexpr int STAGE = 2 * IO::BYTES + 2 * LT * (int)sizeof(float);       // Q | dO | lse (log2 domain) | delta
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const uint64_t seed = drop_p > 0.f ? resolve_seed(seed_arg) : 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int nkb = (Tk + LT - 1) / LT;
  const int bh = blockIdx.x / nkb, b = bh / H, h = bh % H;
  const int key0 = (blockIdx.x % nkb) * LT;
  const int key = key0 + wave * 16 + r;                                     // this lane's key column
  const uint8_t* mb = mask != nullptr ? mask + (size_t)b * Tk : nullptr;
  const uint64_t live = live_keys(mb, key0, Tk, lane);
  if (live == 0) {                       // every key of the block masked: zero gradients (outputs are fully overwritten)
    for (int idx = tid; idx < LT * (DH / 4); idx += NTH) {
      const int row = key0 + idx / (DH / 4), c = idx % (DH / 4);
      if (row < Tk) {
        *(uint2*)(dkp + ((size_t)b * Tk + row) * lddk + h * DH + 4 * c) = make_uint2(0, 0);
        *(uint2*)(dvp + ((size_t)b * Tk + row) * lddv + h * DH + 4 * c) = make_uint2(0, 0);
      }
    }
    return;
  }
  const bool klive = (live >> (wave * 16 + r)) & 1;
  uint4 kf[KK], vf[KK];
  {
    const size_t kr = (size_t)b * Tk + min(key, Tk - 1);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      kf[kk] = *(const uint4*)(kp + kr * ldk + h * DH + (4 * kk + g) * 8);
      vf[kk] = *(const uint4*)(vp + kr * ldv + h * DH + (4 * kk + g) * 8);
    }
  }
  const uint16_t* qb = qp + (size_t)b * Tq * ldq + h * DH;
  const uint16_t* db = dop + (size_t)b * Tq * ldo + h * DH;
  const float* lb = lse + ((size_t)b * H + h) * Tq;
  const float* deb = delta + ((size_t)b * H + h) * Tq;
  uint4 rq[IO::IT], rd[IO::IT];
  float rs = 0.f;                        // threads 0..63: lse row, 64..127: delta row of the next tile
  auto fetch = [&](int t0) {
    IO::load(rq, qb, ldq, t0, Tq, tid);
    IO::load(rd, db, ldo, t0, Tq, tid);
    const int i = t0 + (tid & 63);
    rs = 0.f;
    if (tid < 128 && i < Tq) rs = tid < 64 ? lb[i] * LOG2E : deb[i];
  };
  auto put = [&](char* st) {
    IO::store(st, rq, tid);
    IO::store(st + IO::BYTES, rd, tid);
    if (tid < 128) ((float*)(st + 2 * IO::BYTES))[tid] = rs;
  };
  fetch(0);
  put(smem);
  __syncthreads();

  const float c2 = scale * LOG2E;
  f32x4 dvt[DT], dkt[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dvt[dt] = dkt[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nqt = (Tq + LT - 1) / LT;
  for (int qt = 0; qt < nqt; ++qt) {
    const char* st = smem + (qt & 1) * STAGE;
    const char* q_lds = st;
    const char* do_lds = st + IO::BYTES;
    const float* lse_s = (const float*)(st + 2 * IO::BYTES);
    const float* del_s = lse_s + LT;
    if (qt + 1 < nqt) fetch((qt + 1) * LT);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      uint32_t pp[4], dd[4];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int lr = 32 * s2 + 16 * half;                                // first local query row of the 16-row block
        f32x4 sc = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = sc;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          const uint4 qf = *(const uint4*)(q_lds + (lr + r) * RS + (4 * kk + g) * 16);
          const uint4 df = *(const uint4*)(do_lds + (lr + r) * RS + (4 * kk + g) * 16);
          sc = T::mfma16(qf, kf[kk], sc);                                  // S[query 4g+j][key r]
          dp = T::mfma16(df, vf[kk], dp);                                  // dP[query][key]
        }
        float pv[4], dv4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int li = lr + 4 * g + j, qi = qt * LT + li;
          const float p = (klive && qi < Tq) ? __builtin_amdgcn_exp2f(__builtin_fmaf(sc[j], c2, -lse_s[li])) : 0.f;
          const float f = drop_p > 0.f ? dropout_factor(drop_p, seed, (((size_t)b * H + h) * Tq + min(qi, Tq - 1)) * (size_t)Tk + min(key, Tk - 1)) : 1.0f;
          pv[j] = p * f;
          dv4[j] = p * (dp[j] * f - del_s[li]);
        }
        pp[2 * half] = pack2<T>(pv[0], pv[1]); pp[2 * half + 1] = pack2<T>(pv[2], pv[3]);
        dd[2 * half] = pack2<T>(dv4[0], dv4[1]); dd[2 * half + 1] = pack2<T>(dv4[2], dv4[3]);
      }
      const uint4 pfrag = make_uint4(pp[0], pp[1], pp[2], pp[3]), dsfrag = make_uint4(dd[0], dd[1], dd[2], dd[3]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        // transposed 4-query x 16-column blocks of dO and Q: rows 32 s2 + 4 g + (r>>2) (+16), columns 16 dt + 4 (r&3)..
        const int off = (32 * s2 + 4 * g + (r >> 2)) * RS + (16 * dt + 4 * (r & 3)) * 2;
        dvt[dt] = T::mfma16(tr_pair(do_lds, off, RS), pfrag, dvt[dt]);      // dV^T[d][key]
        dkt[dt] = T::mfma16(tr_pair(q_lds, off, RS), dsfrag, dkt[dt]);      // dK^T[d][key]
      }
    }
    if (qt + 1 < nqt) put(smem + ((qt + 1) & 1) * STAGE);
    __syncthreads();
  }
  if (key < Tk) {
    uint16_t* dvr = dvp + ((size_t)b * Tk + key) * lddv + h * DH + 4 * g;
    uint16_t* dkr = dkp + ((size_t)b * Tk + key) * lddk + h * DH + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      *(uint2*)(dvr + 16 * dt) = make_uint2(pack2<T>(dvt[dt][0], dvt[dt][1]), pack2<T>(dvt[dt][2], dvt[dt][3]));
      *(uint2*)(dkr + 16 * dt) = make_uint2(pack2<T>(dkt[dt][0] * scale, dkt[dt][1] * scale), pack2<T>(dkt[dt][2] * scale, dkt[dt][3] * scale));
    }
  }
}

// Pass 2: dQ of 64 queries (a wave owns 16: lane r = query, registers = keys 4 g + j of each 16-key block).
template <typename T, int DH>
__global__ void __launch_bounds__(NTH) attn_long_bwd_q_kernel(const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
                                                              const uint16_t* __restrict__ vp, const uint8_t* __restrict__ mask,
                                                              const uint16_t* __restrict__ dop, const float* __restrict__ lse,
                                                              const float* __restrict__ delta, uint16_t* __restrict__ dqp, int H, int Tq,
                                                              int Tk, int ldq, int ldk, int ldv, int ldo, int lddq, float scale,
                                                              float drop_p, uint64_t seed_arg) {
  using IO = TileIO<DH>;
  constexpr int KK = DH / 32, DT = DH / 16, RS = IO::RS;
  __shared__ __attribute__((aligned(16))) char smem[4 * IO::BYTES];     // K0 V0 | K1 V1
  const uint64_t seed = drop_p > 0.f ? resolve_seed(seed_arg) : 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int nqb = (Tq + LT - 1) / LT;
  const int bh = blockIdx.x / nqb, b = bh / H, h = bh % H;
  const int qi = (blockIdx.x % nqb) * LT + wave * 16 + r;                  // this lane's query column
  const bool qlive = qi < Tq;
  const uint16_t* kb = kp + (size_t)b * Tk * ldk + h * DH;
  const uint16_t* vb = vp + (size_t)b * Tk * ldv + h * DH;
  const uint8_t* mb = mask != nullptr ? mask + (size_t)b * Tk : nullptr;
  uint4 qf[KK], df[KK];
  float l2 = 0.f, dl = 0.f;
  {
    const size_t qr = (size_t)b * Tq + min(qi, Tq - 1);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      qf[kk] = *(const uint4*)(qp + qr * ldq + h * DH + (4 * kk + g) * 8);
      df[kk] = *(const uint4*)(dop + qr * ldo + h * DH + (4 * kk + g) * 8);
    }
    if (qlive) {
      l2 = lse[((size_t)b * H + h) * Tq + qi] * LOG2E;
      dl = delta[((size_t)b * H + h) * Tq + qi];
    }
  }
  uint4 kr[IO::IT], vr[IO::IT];
  uint64_t live = live_keys(mb, 0, Tk, lane);
  if (live) {
    IO::load(kr, kb, ldk, 0, Tk, tid);
    IO::load(vr, vb, ldv, 0, Tk, tid);
    IO::store(smem, kr, tid);
    IO::store(smem + IO::BYTES, vr, tid);
  }
  __syncthreads();

  const float c2 = scale * LOG2E;
  const size_t drow = (((size_t)b * H + h) * Tq + min(qi, Tq - 1)) * (size_t)Tk;
  f32x4 dqt[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dqt[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nkt = (Tk + LT - 1) / LT;
  for (int kt = 0; kt < nkt; ++kt) {
    const char* k_lds = smem + (kt & 1) * 2 * IO::BYTES;
    const char* v_lds = k_lds + IO::BYTES;
    uint64_t live_next = 0;
    if (kt + 1 < nkt) {
      live_next = live_keys(mb, (kt + 1) * LT, Tk, lane);
      if (live_next) {
        IO::load(kr, kb, ldk, (kt + 1) * LT, Tk, tid);
        IO::load(vr, vb, ldv, (kt + 1) * LT, Tk, tid);
      }
    }
    if (live) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        uint32_t dd[4];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int lk = 32 * s2 + 16 * half;                              // first local key of the 16-key block
          f32x4 sc = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = sc;
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) {
            const uint4 kf = *(const uint4*)(k_lds + (lk + r) * RS + (4 * kk + g) * 16);
            const uint4 vf = *(const uint4*)(v_lds + (lk + r) * RS + (4 * kk + g) * 16);
            sc = T::mfma16(kf, qf[kk], sc);                                // S^T[key 4g+j][query r]
            dp = T::mfma16(vf, df[kk], dp);
          }
          float dv4[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int lj = lk + 4 * g + j;
            const bool kl = qlive && ((live >> lj) & 1);
            const float p = kl ? __builtin_amdgcn_exp2f(__builtin_fmaf(sc[j], c2, -l2)) : 0.f;
            const float f = drop_p > 0.f ? dropout_factor(drop_p, seed, drow + min(kt * LT + lj, Tk - 1)) : 1.0f;
            dv4[j] = p * (dp[j] * f - dl);
          }
          dd[2 * half] = pack2<T>(dv4[0], dv4[1]); dd[2 * half + 1] = pack2<T>(dv4[2], dv4[3]);
        }
        const uint4 dsfrag = make_uint4(dd[0], dd[1], dd[2], dd[3]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          dqt[dt] = T::mfma16(tr_pair(k_lds, (32 * s2 + 4 * g + (r >> 2)) * RS + (16 * dt + 4 * (r & 3)) * 2, RS), dsfrag, dqt[dt]);
      }
    }
    if (live_next) {
      char* kn = smem + ((kt + 1) & 1) * 2 * IO::BYTES;
      IO::store(kn, kr, tid);
      IO::store(kn + IO::BYTES, vr, tid);
    }
    __syncthreads();
    live = live_next;
  }
  if (qlive) {
    uint16_t* dqr = dqp + ((size_t)b * Tq + qi) * lddq + h * DH + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      *(uint2*)(dqr + 16 * dt) = make_uint2(pack2<T>(dqt[dt][0] * scale, dqt[dt][1] * scale), pack2<T>(dqt[dt][2] * scale, dqt[dt][3] * scale));
  }
}

template <typename T, int DH>
int launch_fwd(const AttnPlan& pl, const AttnFwdProblem& p, hipStream_t s) {
  hipLaunchKernelGGL((attn_long_fwd_kernel<T, DH>), dim3(pl.grid[0]), dim3(pl.block), 0, s, (const uint16_t*)p.q, (const uint16_t*)p.k,
                     (const uint16_t*)p.v, p.mask, (uint16_t*)p.out, p.lse, p.H, p.Tq, p.Tk, p.ldq, p.ldk, p.ldv, p.ldo,
                     1.0f / sqrtf((float)p.dh), p.dropout_p, p.seed);
  VMC_CHECK_LAUNCH();
  return 0;
}

template <typename T, int DH>
int launch_bwd(const AttnPlan& pl, const AttnBwdProblem& p, hipStream_t s) {
  const uint16_t *q = (const uint16_t*)p.q, *k = (const uint16_t*)p.k, *v = (const uint16_t*)p.v, *dout = (const uint16_t*)p.dout;
  const float scale = 1.0f / sqrtf((float)p.dh);
  float* delta = (float*)p.workspace;
  hipLaunchKernelGGL((attn_long_delta_kernel<T, DH>), dim3(pl.grid[0]), dim3(pl.block), 0, s, (const uint16_t*)p.out, dout, delta, p.H,
                     p.Tq, p.ldo, (size_t)p.B * p.H * p.Tq);
  hipLaunchKernelGGL((attn_long_bwd_kv_kernel<T, DH>), dim3(pl.grid[1]), dim3(pl.block), 0, s, q, k, v, p.mask, dout, p.lse, delta,
                     (uint16_t*)p.dk, (uint16_t*)p.dv, p.H, p.Tq, p.Tk, p.ldq, p.ldk, p.ldv, p.ldo, p.lddk, p.lddv, scale, p.dropout_p,
                     p.seed);
  hipLaunchKernelGGL((attn_long_bwd_q_kernel<T, DH>), dim3(pl.grid[2]), dim3(pl.block), 0, s, q, k, v, p.mask, dout, p.lse, delta,
                     (uint16_t*)p.dq, p.H, p.Tq, p.Tk, p.ldq, p.ldk, p.ldv, p.ldo, p.lddq, scale, p.dropout_p, p.seed);
  VMC_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// The executors of attn_route.h's ATTN_LONG_FWD / ATTN_LONG_BWD plans (declared in common.h).
int attn_long_fwd(const AttnPlan& pl, const AttnFwdProblem& p, hipStream_t s) {
  if (p.dtype16 == VMC_BF16) return pl.dh == 64 ? launch_fwd<BF16, 64>(pl, p, s) : launch_fwd<BF16, 96>(pl, p, s);
  return pl.dh == 64 ? launch_fwd<F16, 64>(pl, p, s) : launch_fwd<F16, 96>(pl, p, s);
}

int attn_long_bwd(const AttnPlan& pl, const AttnBwdProblem& p, hipStream_t s) {
  if (p.dtype16 == VMC_BF16) return pl.dh == 64 ? launch_bwd<BF16, 64>(pl, p, s) : launch_bwd<BF16, 96>(pl, p, s);
  return pl.dh == 64 ? launch_bwd<F16, 64>(pl, p, s) : launch_bwd<F16, 96>(pl, p, s);
}
