// K17 -- batch assembly from a device-resident embedding store (gfx950): what HDF5VideoDataset.__getitem__ + collate_fn_pad do on
// the host (TFAM/data/dataset.py:38-51, 76-112), for videos whose token rows already sit in device memory.
//
// ONE launch writes everything a TFAM step reads from its batch: both padded token tensors, both masks, the label rows and the two
// batch lengths.  The step it feeds is launch bound (a captured step is ~1 ms of ~4 us launches), so the work is not split by output.
//
// Pure data movement, ~4 MB at the reference batch (8 clips x 64 rows x 512 floats x 2 streams, read + written): no LDS, no reuse.
//   grid = (ceil(max T_out / GC_ROWS), B, n_streams), 256 threads.  A workgroup owns GC_ROWS = 4 consecutive output rows of one clip
//   of one stream: 64 x 8 x 2 = 256 workgroups at the reference batch, one per CU.  Rows t < length are copied, the others are
//   written as zeros: every output element is written on every call, so a graph replay never sees the previous batch.
//   16 bytes per lane where D % 4 == 0 and both bases are 16-byte aligned (the host decides per stream), otherwise 4 bytes.
//   The workgroups with blockIdx.x == 0 also write their clip's mask row, those of stream 0 the label row.
//   Thread 0 of workgroup (0, 0, 0) loops over the B indices for max_len and status, after its share of the copy: no atomics, the
//   same value on every replay.
//
// BOUNDS.  `index` is device memory the host cannot validate: every use of an index value i is guarded by 0 <= i < n_videos BEFORE
// offset[i], length[i] or labels[i] is addressed; a bad index gives an empty clip (zero rows, zero mask, zero labels).  The length
// is clamped into [0, T_out], so no row beyond the output or (for a store whose offset / length are consistent) the clip is touched.
#include "common.h"

#define GC_ROWS 4

struct GcStream {
  const float* rows;
  const long long* offset;
  const int* length;
  float* out;
  uint8_t* mask;
  int* max_len;
  int T_out;
  int vec;        // 16-byte path: D % 4 == 0, rows and out 16-byte aligned
};
struct GcArgs {
  GcStream s[2];
  const int* index;
  const float* labels;
  float* labels_out;
  int* status;
  long long n_videos;
  int n_streams, B, D, C;
};

__global__ void __launch_bounds__(256) gather_clips_kernel(const GcArgs a) {
  const int z = blockIdx.z, b = blockIdx.y;
  const GcStream st = z == 0 ? a.s[0] : a.s[1];        // selects, not a dynamically indexed copy of the arguments
  const int t0 = blockIdx.x * GC_ROWS;
  const int T_out = st.T_out;
  const int D = a.D;
  if (t0 < T_out) {                                  // the grid is sized for the longer stream
    const long long i = a.index[b];
    const bool ok = i >= 0 && i < a.n_videos;
    int len = 0;
    long long first = 0;
    if (ok) {
      len = st.length[i];
      first = st.offset[i];
      len = len < 0 ? 0 : (len > T_out ? T_out : len);
    }
    const int t1 = t0 + GC_ROWS < T_out ? t0 + GC_ROWS : T_out;
    const int nrow = t1 - t0;
    float* dst = st.out + ((size_t)b * T_out + t0) * D;                 // rows t0 .. t1-1 of clip b are contiguous
    const float* src = st.rows + ((size_t)first + t0) * D;              // dereferenced only below `len`
    const int ncopy = len - t0;                                         // rows of this group that are real (may be <= 0)
    if (st.vec) {
      const int D4 = D >> 2;
      const int n = nrow * D4;
      const int nreal = ncopy > 0 ? (ncopy < nrow ? ncopy : nrow) * D4 : 0;
      const float4* s4 = (const float4*)src;
      float4* d4 = (float4*)dst;
      for (int e = threadIdx.x; e < n; e += 256) d4[e] = e < nreal ? s4[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      const int n = nrow * D;
      const int nreal = ncopy > 0 ? (ncopy < nrow ? ncopy : nrow) * D : 0;
      for (int e = threadIdx.x; e < n; e += 256) dst[e] = e < nreal ? src[e] : 0.f;
    }
    if (blockIdx.x == 0) {
      uint8_t* m = st.mask + (size_t)b * T_out;
      for (int t = threadIdx.x; t < T_out; t += 256) m[t] = t < len ? 1 : 0;
      if (z == 0 && a.labels != nullptr) {
        const float* lsrc = a.labels + (size_t)(ok ? i : 0) * a.C;
        float* ldst = a.labels_out + (size_t)b * a.C;
        for (int c = threadIdx.x; c < a.C; c += 256) ldst[c] = ok ? lsrc[c] : 0.f;
      }
    }
  }
  if (blockIdx.x == 0 && b == 0 && z == 0 && threadIdx.x == 0) {
    int mx0 = 1, mx1 = 1, bits = 0;
    for (int k = 0; k < a.B; ++k) {
      const long long i = a.index[k];
      if (i < 0 || i >= a.n_videos) {
        bits |= 1;
        continue;
      }
      int len = a.s[0].length[i];
      len = len < 0 ? 0 : len;                                          // as the copy path: a negative length counts as 0
      if (len > a.s[0].T_out) bits |= 2, len = a.s[0].T_out;
      mx0 = len > mx0 ? len : mx0;
      if (a.n_streams > 1) {
        len = a.s[1].length[i];
        len = len < 0 ? 0 : len;
        if (len > a.s[1].T_out) bits |= 2, len = a.s[1].T_out;
        mx1 = len > mx1 ? len : mx1;
      }
    }
    if (a.s[0].max_len != nullptr) *a.s[0].max_len = mx0;
    if (a.n_streams > 1 && a.s[1].max_len != nullptr) *a.s[1].max_len = mx1;
    if (a.status != nullptr && bits != 0) *a.status |= bits;
  }
}

extern "C" int vmc_gather_clips(const vmc_clip_stream* streams, int n_streams, const int* index, int B, long long n_videos, int D,
                                const float* labels, float* labels_out, int C, int* status, void* stream) {
  if (!streams || !index || n_streams < 1 || n_streams > 2 || B <= 0 || D <= 0 || n_videos <= 0) return VMC_E_ARG;
  if (labels != nullptr && (!labels_out || C <= 0)) return VMC_E_ARG;
  if (B > 65535) return VMC_E_SHAPE;
  GcArgs a = {};
  int T_max = 0;
  for (int q = 0; q < n_streams; ++q) {
    const vmc_clip_stream& s = streams[q];
    if (!s.rows || !s.offset || !s.length || !s.out || !s.mask || s.T_out <= 0) return VMC_E_ARG;
    if ((long long)GC_ROWS * D > 0x7FFFFFFFll / 2) return VMC_E_SHAPE;          // per-group element counts are ints
    const int vec = D % 4 == 0 && (((uintptr_t)s.rows | (uintptr_t)s.out) & 15) == 0;
    a.s[q] = GcStream{s.rows, s.offset, s.length, s.out, s.mask, s.max_len, s.T_out, vec};
    T_max = s.T_out > T_max ? s.T_out : T_max;
  }
  a.index = index;
  a.labels = labels;
  a.labels_out = labels_out;
  a.status = status;
  a.n_videos = n_videos;
  a.n_streams = n_streams;
  a.B = B;
  a.D = D;
  a.C = C;
  const dim3 grid((unsigned)((T_max + GC_ROWS - 1) / GC_ROWS), (unsigned)B, (unsigned)n_streams);
  hipLaunchKernelGGL(gather_clips_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  VMC_CHECK_LAUNCH();
  return 0;
}
