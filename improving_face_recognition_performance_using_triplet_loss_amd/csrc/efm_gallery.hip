// Device-resident face gallery: fused cosine scan + top-k / threshold selection on the matrix cores, and the merge of the per-tile
// candidate lists (ref: Feature.hpp:295-343 Compare_Face_From_DB top-k, 345-392 the in-memory argmax, 763-804 Compare_Face_Person /
// Compare_Face_DB best identity).
//
// Gallery layout: row i = g_i / |g_i| in fp32 or bf16, row stride ldg a multiple of 32 elements, columns d..ldg-1 zero
// (efm_gallery_pack writes it).  The score is s = <q, g_i> / |q|.
//
// Selection rule (scan, block merge and final merge alike): a candidate is kept when s >= sim_th; candidates rank by score
// descending, then by gallery row ascending; empty slots are (-inf, -1, -1); a query of zero norm matches nothing.  With labels the
// list holds distinct labels, each at its best row.  Because the rule is a total order, inserting the candidates of any partition of
// the gallery in any order yields the same list, and the top-k of a union is contained in the union of the parts' top-k (for labels:
// a label of the global top-k has its best row in some part, where fewer than k labels can beat it) — so tile -> block -> merge is
// exact.
//
// Scan block = 4 waves x one tile of 16 queries (the MFMA's N) held in LDS, cast to the gallery dtype once.  Each wave streams
// groups of 64 gallery rows (4 MFMA row tiles of 16) straight from global memory into the A operand: lane l of row tile r holds row
// 16 r + (l & 15), columns 8 (l >> 4) .. +7 of each 32-column step (bf16, v_mfma_f32_16x16x32_bf16) or 4 (l >> 4) .. +3 of each
// 16-column step (fp32, v_mfma_f32_16x16x4_f32, the four k-steps of one float4 taken in a permuted but A/B-consistent order).  The
// accumulator gives lane l the scores of query l & 15 against rows 16 r + 4 (l >> 4) + j.  Each lane keeps the admission threshold of
// its query (sim_th until the list is full, then the k-th score), so the common case is one compare per score and one ballot per
// group; the few scores that pass are inserted one at a time into the wave's sorted per-query list in LDS by all 64 lanes at once.
// At the end the four wave lists of each query are merged in LDS and the block writes one list of k candidates per (query, tile).
// Blocks are numbered query tile fastest, so the query tiles that share a gallery tile run together and re-read it from L2 / MALL.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <type_traits>

#include "efm_common.h"

namespace {

constexpr int QT = 16;              // queries per scan block
constexpr int WAVES = 4;
constexpr int GROUP = 64;           // gallery rows per wave iteration
constexpr int TARGET_BLOCKS = 1024; // scan blocks aimed at per launch (4 per CU)
constexpr int KMAX = 32;
constexpr int DMAX = 1024;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct Cand {
  float s;
  int32_t i;
  int32_t l;
};

inline int qtiles(int nq) { return (nq + QT - 1) / QT; }
// Gallery tiles per scan (= candidate lists per query per workspace slot): fixed by nq, so every slot of one merge has the same layout.
inline int gtiles(int nq) { return (TARGET_BLOCKS + qtiles(nq) - 1) / qtiles(nq); }

__device__ __forceinline__ bool better(float s, int i, float es, int ei) { return s > es || (s == es && i < ei); }

__device__ __forceinline__ float bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
__device__ __forceinline__ int bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

// Inserts the wave-uniform candidate (s, row, lab) into the sorted list (ls, li, ll)[0..cnt) of capacity k, all 64 lanes at once
// (lane j holds entry j; k <= 32).  cnt is wave-uniform and updated.
__device__ void list_insert(float* ls, int* li, int* ll, int& cnt, int k, bool by_label, float s, int row, int lab, int lane) {
  const bool have = lane < cnt;
  float es = -INFINITY;
  int ei = INT_MAX, el = 0;
  if (have) {
    es = ls[lane];
    ei = li[lane];
    el = ll[lane];
  }
  const int pos = __popcll(__ballot(have && !better(s, row, es, ei)));  // entries that rank before the new one (a prefix)
  int end;                                                              // entries [pos, end) move down one slot
  bool grow = true;
  if (by_label) {
    const unsigned long long m = __ballot(have && el == lab);
    if (m) {
      const int mpos = __ffsll((long long)m) - 1;
      if (mpos < pos) return;  // this identity already holds a better row
      end = mpos;              // its old row leaves, the rows in between move down
      grow = false;
    } else {
      end = cnt < k ? cnt : k - 1;
    }
  } else {
    end = cnt < k ? cnt : k - 1;
  }
  if (pos >= k) return;
  if (lane >= pos && lane < end) {
    ls[lane + 1] = es;
    li[lane + 1] = ei;
    ll[lane + 1] = el;
  }
  if (lane == pos) {
    ls[pos] = s;
    li[pos] = row;
    ll[pos] = lab;
  }
  if (grow && cnt < k) ++cnt;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Every lane offers one candidate to one wave-uniform list; those at or above the list's threshold go in, lowest lane first.
__device__ void offer(float* ls, int* li, int* ll, int& cnt, float& thr, float th0, int k, bool by_label, float s, int row, int lab,
                      int lane) {
  unsigned long long m = __ballot(s >= thr);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    list_insert(ls, li, ll, cnt, k, by_label, bcast(s, src), bcast(row, src), bcast(lab, src), lane);
    if (cnt == k) thr = fmaxf(th0, ls[k - 1]);
    m &= ~(1ull << src);
    m &= __ballot(s >= thr);
  }
}

template <bool BF16>
__global__ void __launch_bounds__(256) gallery_scan_k(const float* __restrict__ query, int nq, int d, int ldq, const void* __restrict__ gallery,
                                                      int n, int ldg, const int32_t* __restrict__ labels, int row_offset, int k, float sim_th,
                                                      Cand* __restrict__ out, int nqt, int T, int rpt) {
  using E = typename std::conditional<BF16, __bf16, float>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int dpad = (d + 31) & ~31;
  const int qld = dpad + 16 / (int)sizeof(E);  // one 16-B slot of row padding against bank conflicts of the B-operand reads
  E* qs = reinterpret_cast<E*>(smem);
  float* ls = reinterpret_cast<float*>(smem + (((size_t)QT * qld * sizeof(E) + 15) & ~(size_t)15));
  int* li = reinterpret_cast<int*>(ls + WAVES * QT * k);
  int* ll = li + WAVES * QT * k;
  int* lcnt = ll + WAVES * QT * k;
  float* qinv = reinterpret_cast<float*>(lcnt + WAVES * QT);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int qt = blockIdx.x % nqt, t = blockIdx.x / nqt;
  const int q0 = qt * QT;
  for (int e = tid; e < QT * dpad; e += 256) {
    const int r = e / dpad, c = e - r * dpad, q = q0 + r;
    qs[r * qld + c] = (E)((q < nq && c < d) ? query[(long)q * ldq + c] : 0.f);
  }
  if (tid < WAVES * QT) lcnt[tid] = 0;
  __syncthreads();
  for (int r = w * 4; r < w * 4 + 4; ++r) {  // 1 / |q| of the query as stored (after the cast)
    float s = 0.f;
    for (int c = lane; c < dpad; c += 64) {
      const float v = (float)qs[r * qld + c];
      s = fmaf(v, v, s);
    }
    s = efm::wave_sum(s);
    if (lane == 0) qinv[r] = (q0 + r < nq && s > 0.f) ? 1.f / sqrtf(s) : 0.f;
  }
  __syncthreads();

  const int fr = lane & 15, fk = lane >> 4;
  const float inv = qinv[fr];
  const float th0 = fmaxf(sim_th, -FLT_MAX);  // -inf (an empty or invalid score) never passes
  float thr = inv > 0.f ? th0 : INFINITY;
  const bool by_label = labels != nullptr;
  const int tile0 = t * rpt, tile1 = min(n, tile0 + rpt);
  float* wls = ls + w * QT * k;
  int* wli = li + w * QT * k;
  int* wll = ll + w * QT * k;

  for (int g0 = tile0 + w * GROUP; g0 < tile1; g0 += WAVES * GROUP) {
    f32x4 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BF16) {
      const __bf16* G = reinterpret_cast<const __bf16*>(gallery);
      for (int kk = 0; kk < dpad; kk += 32) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(qs + fr * qld + kk + 8 * fk);
        bf16x8 a[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = g0 + r * 16 + fr;
          if (row < tile1) {
            a[r] = *reinterpret_cast<const bf16x8*>(G + (long)row * ldg + kk + 8 * fk);
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) a[r][j] = (__bf16)0.f;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[r], b, acc[r], 0, 0, 0);
      }
    } else {
      const float* G = reinterpret_cast<const float*>(gallery);
      for (int kk = 0; kk < dpad; kk += 16) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(qs + fr * qld + kk + 4 * fk);
        f32x4 a[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = g0 + r * 16 + fr;
          a[r] = row < tile1 ? *reinterpret_cast<const f32x4*>(G + (long)row * ldg + kk + 4 * fk) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r][j], b[j], acc[r], 0, 0, 0);
      }
    }
    bool any = false;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = g0 + r * 16 + 4 * fk + j;
        const float s = (row < tile1 && inv > 0.f) ? acc[r][j] * inv : -INFINITY;
        acc[r][j] = s;
        any |= s >= thr;
      }
    if (__ballot(any) == 0) continue;  // the common case
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned long long m = __ballot(acc[r][j] >= thr);
        while (m) {
          const int src = __ffsll((long long)m) - 1;
          const int q = src & 15, row = g0 + r * 16 + 4 * (src >> 4) + j;
          const float s = bcast(acc[r][j], src);
          const int lab = by_label ? labels[row] : -1;
          int cnt = lcnt[w * QT + q];
          list_insert(wls + q * k, wli + q * k, wll + q * k, cnt, k, by_label, s, row, lab, lane);
          if (lane == 0) lcnt[w * QT + q] = cnt;
          if (cnt == k) {
            const float nt = fmaxf(th0, wls[q * k + k - 1]);
            if (fr == q) thr = nt;
          }
          m &= ~(1ull << src);
          m &= __ballot(acc[r][j] >= thr);
        }
      }
  }
  __syncthreads();

  // the four wave lists of query q -> wave 0's list, then out[(q, t)] (wave w does queries 4 w .. 4 w + 3)
  for (int r = w * 4; r < w * 4 + 4; ++r) {
    float* dls = ls + r * k;
    int* dli = li + r * k;
    int* dll = ll + r * k;
    int cnt = lcnt[r];
    float th = cnt == k ? fmaxf(th0, dls[k - 1]) : th0;
    for (int sw = 1; sw < WAVES; ++sw) {
      const int base = (sw * QT + r) * k, c2 = lcnt[sw * QT + r];
      float s = -INFINITY;
      int row = 0, lab = 0;
      if (lane < c2) {
        s = ls[base + lane];
        row = li[base + lane];
        lab = ll[base + lane];
      }
      offer(dls, dli, dll, cnt, th, th0, k, by_label, s, row, lab, lane);
    }
    const int qg = q0 + r;
    if (qg < nq && lane < k) {
      Cand c{-INFINITY, -1, -1};
      if (lane < cnt) c = Cand{dls[lane], dli[lane] + row_offset, dll[lane]};
      out[((long)qg * T + t) * k + lane] = c;
    }
  }
}

// One block per query: each wave folds a quarter of the query's candidate lists (all slots) into its own LDS list, wave 0 folds the
// other three into its own and writes the result.
__global__ void __launch_bounds__(256) gallery_merge_k(const Cand* __restrict__ ws, int nslots, int nq, int T, int k, int by_label,
                                                       float* __restrict__ top_s, int32_t* __restrict__ top_i, int32_t* __restrict__ top_l) {
  __shared__ float ls[WAVES * KMAX];
  __shared__ int li[WAVES * KMAX], ll[WAVES * KMAX], lcnt[WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, q = blockIdx.x;
  const long per = (long)T * k;
  int cnt = 0;
  float thr = -FLT_MAX;
  for (int slot = 0; slot < nslots; ++slot) {
    const Cand* c = ws + ((long)slot * nq + q) * per;
    for (long b = (long)w * 64; b < per; b += 4 * WAVES * 64) {
      Cand x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // four independent loads in flight per lane
        const long e = b + (long)u * WAVES * 64 + lane;
        x[u] = e < per ? c[e] : Cand{-INFINITY, -1, -1};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) offer(ls + w * KMAX, li + w * KMAX, ll + w * KMAX, cnt, thr, -FLT_MAX, k, by_label, x[u].s, x[u].i, x[u].l, lane);
    }
  }
  if (lane == 0) lcnt[w] = cnt;
  __syncthreads();
  if (w != 0) return;
  for (int sw = 1; sw < WAVES; ++sw) {
    const int c2 = lcnt[sw];
    float s = -INFINITY;
    int row = 0, lab = 0;
    if (lane < c2) {
      s = ls[sw * KMAX + lane];
      row = li[sw * KMAX + lane];
      lab = ll[sw * KMAX + lane];
    }
    offer(ls, li, ll, cnt, thr, -FLT_MAX, k, by_label, s, row, lab, lane);
  }
  if (lane < k) {
    const bool h = lane < cnt;
    top_s[(long)q * k + lane] = h ? ls[lane] : -INFINITY;
    top_i[(long)q * k + lane] = h ? li[lane] : -1;
    if (top_l) top_l[(long)q * k + lane] = h ? ll[lane] : -1;
  }
}

// dst row i = x_i / |x_i| in the gallery dtype, columns d..ldd-1 zero; one wave per row.
template <bool BF16>
__global__ void __launch_bounds__(256) gallery_pack_k(const float* __restrict__ x, int rows, int d, int ldx, void* __restrict__ dst, int ldd) {
  using E = typename std::conditional<BF16, __bf16, float>::type;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (long)row * ldx;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s = fmaf(xr[c], xr[c], s);
  s = efm::wave_sum(s);
  const float nrm = sqrtf(s);
  E* o = reinterpret_cast<E*>(dst) + (long)row * ldd;
  for (int c = lane; c < ldd; c += 64) o[c] = (E)((c < d && nrm > 0.f) ? xr[c] / nrm : 0.f);
}

size_t scan_lds_bytes(int d, int k, bool bf16) {
  const int dpad = (d + 31) & ~31, es = bf16 ? 2 : 4;
  const size_t q = ((size_t)QT * (dpad + 16 / es) * es + 15) & ~(size_t)15;
  return q + (size_t)WAVES * QT * k * 12 + WAVES * QT * 4 + QT * 4;
}

}  // namespace

size_t efm_gallery_workspace_bytes(int nq, int nslots, int k) {
  if (nq < 1 || nslots < 1 || k < 1 || k > KMAX) return 0;
  return (size_t)nslots * nq * gtiles(nq) * k * sizeof(Cand);
}

int efm_gallery_pack(const float* x, int rows, int d, int ldx, void* dst, int bf16, int ldd, void* stream) {
  EFM_REQUIRE(x && dst, "gallery_pack: null pointer");
  EFM_REQUIRE(rows >= 1 && d >= 1 && d <= DMAX, "gallery_pack: rows = %d, d = %d (need rows >= 1, 1 <= d <= %d)", rows, d, DMAX);
  EFM_REQUIRE(ldx >= d, "gallery_pack: ldx = %d < d = %d", ldx, d);
  EFM_REQUIRE(ldd >= d && ldd % 32 == 0, "gallery_pack: ldd = %d must be a multiple of 32 and >= d = %d", ldd, d);
  EFM_REQUIRE(((uintptr_t)dst & 15) == 0, "gallery_pack: dst must be 16-byte aligned");
  const dim3 grid((rows + 3) / 4);
  if (bf16)
    hipLaunchKernelGGL(gallery_pack_k<true>, grid, dim3(256), 0, (hipStream_t)stream, x, rows, d, ldx, dst, ldd);
  else
    hipLaunchKernelGGL(gallery_pack_k<false>, grid, dim3(256), 0, (hipStream_t)stream, x, rows, d, ldx, dst, ldd);
  return efm::check_launch("gallery_pack");
}

int efm_gallery_scan(const float* query, int nq, int d, int ldq, const void* gallery, int bf16, int n, int ldg, const int32_t* labels,
                     int64_t row_offset, int k, float sim_th, void* workspace, int slot, void* stream) {
  EFM_REQUIRE(query && gallery && workspace, "gallery_scan: null pointer");
  EFM_REQUIRE(k >= 1 && k <= KMAX, "gallery_scan: k = %d outside 1..%d", k, KMAX);
  EFM_REQUIRE(nq >= 1 && n >= 1 && d >= 1 && d <= DMAX, "gallery_scan: nq = %d, n = %d, d = %d (need nq, n >= 1, 1 <= d <= %d)", nq, n, d, DMAX);
  EFM_REQUIRE(ldq >= d, "gallery_scan: ldq = %d < d = %d", ldq, d);
  EFM_REQUIRE(ldg % 32 == 0 && ldg >= ((d + 31) & ~31), "gallery_scan: ldg = %d must be a multiple of 32 and >= pad32(d)", ldg);
  EFM_REQUIRE(((uintptr_t)gallery & 15) == 0, "gallery_scan: gallery must be 16-byte aligned");
  EFM_REQUIRE(!isnan(sim_th), "gallery_scan: sim_th is NaN");
  EFM_REQUIRE(row_offset >= 0 && row_offset + n <= INT32_MAX, "gallery_scan: row_offset + n must fit in int32");
  EFM_REQUIRE(slot >= 0, "gallery_scan: slot = %d < 0", slot);
  const int nqt = qtiles(nq), T = gtiles(nq);
  const int rpt = (int)(efm::cdiv(efm::cdiv(n, T), GROUP) * GROUP);
  Cand* out = reinterpret_cast<Cand*>(workspace) + (size_t)slot * nq * T * k;
  const size_t lds = scan_lds_bytes(d, k, bf16 != 0);
  const dim3 grid((unsigned)nqt * T);
  if (bf16) {
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)gallery_scan_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(gallery_scan_k<true>, grid, dim3(256), lds, (hipStream_t)stream, query, nq, d, ldq, gallery, n, ldg, labels,
                       (int)row_offset, k, sim_th, out, nqt, T, rpt);
  } else {
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)gallery_scan_k<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(gallery_scan_k<false>, grid, dim3(256), lds, (hipStream_t)stream, query, nq, d, ldq, gallery, n, ldg, labels,
                       (int)row_offset, k, sim_th, out, nqt, T, rpt);
  }
  return efm::check_launch("gallery_scan");
}

int efm_gallery_merge(const void* workspace, int nslots, int nq, int k, int by_label, float* top_scores, int32_t* top_index,
                      int32_t* top_label, void* stream) {
  EFM_REQUIRE(workspace && top_scores && top_index, "gallery_merge: null pointer");
  EFM_REQUIRE(k >= 1 && k <= KMAX, "gallery_merge: k = %d outside 1..%d", k, KMAX);
  EFM_REQUIRE(nq >= 1 && nslots >= 1, "gallery_merge: nq = %d, nslots = %d (need >= 1)", nq, nslots);
  hipLaunchKernelGGL(gallery_merge_k, dim3(nq), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const Cand*>(workspace), nslots, nq,
                     gtiles(nq), k, by_label, top_scores, top_index, top_label);
  return efm::check_launch("gallery_merge");
}
