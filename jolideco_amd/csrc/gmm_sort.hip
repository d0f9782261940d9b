// Counting sort by component for the 8x8 GMM patch prior: of the patches by their arg-max component (bucketed backward
// pass, gmm.hip) and of the screen's candidate records (gmm_screen.hip).  LDS histograms per block, a scan over the
// blocks per bin, no global atomics; buckets are padded to 32 slots; the order inside a bucket influences no result.
#include "gmm_internal.h"

namespace jd {

// component of element n, or a negative number if it takes no part (-1: filtered patch)
__device__ __forceinline__ int bucket_key(const GmmBucketArgs& a, int n) {
  if (a.seg_cnt && !(a.rec_ub[n] >= a.lfinal[a.rec_n[n]] - a.margin)) return -2;  // stale record
  if (a.dense_mark && a.dense_mark[a.rec_n[n]] != 0) return -2;
  return a.argmax[n];
}
// number of elements of chunk c that are in use
__device__ __forceinline__ int bucket_chunk_size(const GmmBucketArgs& a, int c) {
  const int left = a.n_end - (a.n_begin + c * a.chunk);
  const int full = left < a.chunk ? left : a.chunk;
  if (!a.seg_cnt) return full;
  const int used = a.seg_cnt[c];  // chunk == record segment
  return used < full ? used : full;
}

// The keys of elements i, i + 256, ... (UN of them; i < size) of a chunk of candidate RECORDS (a.seg_cnt != nullptr) with
// every load unconditional and the independent ones issued together: record -> (patch, bound, component), then the
// patch's final bound.  Through bucket_key, element by element, a thread ran three dependent round trips per record
// (patch, final bound, then -- under the test -- the component).  key = -3: no element (past the chunk's used slots).
template <int UN>
__device__ __forceinline__ void record_keys(const GmmBucketArgs& a, int base, int i, int size, int (&key)[UN], int (&patch)[UN]) {
  int n[UN], kk[UN];
  float ub[UN], lf[UN];
#pragma unroll
  for (int u = 0; u < UN; ++u) n[u] = base + (i + 256 * u < size ? i + 256 * u : i);
#pragma unroll
  for (int u = 0; u < UN; ++u) patch[u] = a.rec_n[n[u]], ub[u] = a.rec_ub[n[u]], kk[u] = a.argmax[n[u]];
#pragma unroll
  for (int u = 0; u < UN; ++u) lf[u] = a.lfinal[patch[u]];
#pragma unroll
  for (int u = 0; u < UN; ++u) {
    bool stale = !(ub[u] >= lf[u] - a.margin);
    if (a.dense_mark) stale = stale || a.dense_mark[patch[u]] != 0;  // (logsumexp screen only)
    key[u] = i + 256 * u < size ? (stale ? -2 : kk[u]) : -3;
  }
}
constexpr int BUCKET_UN = 2;

// Each block walks over chunks blockIdx.x, blockIdx.x + gridDim.x, ... and touches the global counters once per
// bin: with one chunk per block the (bins x blocks) global atomics on a few hundred addresses were the cost.
__global__ __launch_bounds__(256) void gmm_bucket_count_kernel(GmmBucketArgs a) {
  extern __shared__ int hist[];
  for (int k = threadIdx.x; k < a.K; k += 256) hist[k] = 0;
  __syncthreads();
  const int n_chunks = (a.n_end - a.n_begin + a.chunk - 1) / a.chunk;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int base = a.n_begin + c * a.chunk, size = bucket_chunk_size(a, c);
    if (a.seg_cnt) {  // (uniform) candidate records: batched loads
      for (int i = threadIdx.x; i < size; i += 256 * BUCKET_UN) {
        int key[BUCKET_UN], patch[BUCKET_UN];
        record_keys<BUCKET_UN>(a, base, i, size, key, patch);
#pragma unroll
        for (int u = 0; u < BUCKET_UN; ++u)
          if (key[u] >= 0) atomicAdd(&hist[key[u]], 1);
      }
      continue;
    }
    for (int i = threadIdx.x; i < size; i += 256) {
      const int k = bucket_key(a, base + i);
      if (k >= 0) atomicAdd(&hist[k], 1);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < a.K; k += 256) a.blk_counts[(size_t)k * gridDim.x + blockIdx.x] = hist[k];
}

// Block k: exclusive prefix over the blocks of bin k's per-block counts (in place) and the bin total.  No global
// atomics anywhere in the sort: with hundreds of blocks hammering a few hundred counters they were its whole cost.
__global__ __launch_bounds__(256) void gmm_bucket_binscan_kernel(GmmBucketArgs a, int n_blk) {
  __shared__ int part[2][256];
  const int k = blockIdx.x;
  const int per = (n_blk + 255) / 256;
  const int b0 = threadIdx.x * per;
  int local = 0;
  int* bin = a.blk_counts + (size_t)k * n_blk;
  for (int b = b0; b < b0 + per && b < n_blk; ++b) local += bin[b];
  int cur = 0;
  part[0][threadIdx.x] = local;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    int v = part[cur][threadIdx.x];
    if ((int)threadIdx.x >= off) v += part[cur][threadIdx.x - off];
    part[cur ^ 1][threadIdx.x] = v;
    cur ^= 1;
    __syncthreads();
  }
  int run = part[cur][threadIdx.x] - local;
  for (int b = b0; b < b0 + per && b < n_blk; ++b) {
    const int v = bin[b];
    bin[b] = run;
    run += v;
  }
  if (threadIdx.x == 255) a.counts[k] = part[cur][255];
}

// The same scan with the thread's counts held in registers (n_blk <= 256 PER): ONE batch of unconditional loads, a wave
// scan by cross-lane moves + the four wave totals through LDS, one batch of stores.  The loop form above runs a load and a
// wait per count, twice (12 dependent round trips at 2040 blocks: 5 us for 1 MB).
template <int PER>
__global__ __launch_bounds__(256) void gmm_bucket_binscan_reg_kernel(GmmBucketArgs a, int n_blk) {
  __shared__ int wave_total[4];
  const int k = blockIdx.x;
  const int per = (n_blk + 255) / 256;
  const int b0 = threadIdx.x * per;
  int* bin = a.blk_counts + (size_t)k * n_blk;
  int vals[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int b = b0 + j;
    const int v = bin[b < n_blk ? b : n_blk - 1];
    vals[j] = (j < per && b < n_blk) ? v : 0;
  }
  int local = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) local += vals[j];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = local;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wave_total[wv] = incl;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wv; ++w) before += wave_total[w];
  int run = before + incl - local;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int b = b0 + j;
    if (j < per && b < n_blk) bin[b] = run;
    run += vals[j];
  }
  if (threadIdx.x == 255) a.counts[k] = before + incl;
}

static void launch_binscan(const GmmBucketArgs& bk, int K, int n_blk, hipStream_t s) {
  const int per = (n_blk + 255) / 256;
  if (per <= 8)
    gmm_bucket_binscan_reg_kernel<8><<<K, 256, 0, s>>>(bk, n_blk);
  else if (per <= 32)
    gmm_bucket_binscan_reg_kernel<32><<<K, 256, 0, s>>>(bk, n_blk);
  else
    gmm_bucket_binscan_kernel<<<K, 256, 0, s>>>(bk, n_blk);
}

// Exclusive scan of the padded bucket sizes, by EVERY block of the scatter kernel for itself (K bin totals: a few hundred
// loads and one LDS scan -- cheaper than the 6.5 us a dependent single-block launch costs); block 0 also publishes the
// offsets for the kernels that follow, raises the overflow flag and ranks the bins for the next screen.
// off[k] (LDS, K + 1 entries) <- offsets; thread t owns a contiguous segment of bins, the 256 segment sums are scanned
// in LDS (Hillis-Steele).
__device__ __forceinline__ void bucket_offsets(const GmmBucketArgs& a, int* off, int* cnt) {
  __shared__ int part[2][256];
  for (int k = threadIdx.x; k < a.K; k += 256) cnt[k] = a.counts[k];
  __syncthreads();
  const int seg = (a.K + 255) / 256;
  const int k0 = threadIdx.x * seg;
  int local = 0;
  for (int k = k0; k < k0 + seg && k < a.K; ++k) local += (cnt[k] + 31) & ~31;
  int cur = 0;
  part[0][threadIdx.x] = local;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    int v = part[cur][threadIdx.x];
    if ((int)threadIdx.x >= o) v += part[cur][threadIdx.x - o];
    part[cur ^ 1][threadIdx.x] = v;
    cur ^= 1;
    __syncthreads();
  }
  int total = part[cur][threadIdx.x] - local;  // exclusive prefix of this thread's segment
  for (int k = k0; k < k0 + seg && k < a.K; ++k) {
    off[k] = total;
    total += (cnt[k] + 31) & ~31;
  }
  if (threadIdx.x == 255) off[a.K] = part[cur][255];
  __syncthreads();
  if (blockIdx.x != 0) return;
  for (int k = threadIdx.x; k <= a.K; k += 256) a.offsets[k] = off[k];
  if (threadIdx.x == 0 && a.flag && off[a.K] > a.slot_cap) __hip_atomic_store(a.flag, a.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (a.korder) {  // bins by size, largest first (ties: lowest index): the visiting order of the next screen
    for (int k = threadIdx.x; k < a.K; k += 256) {
      const int ck = cnt[k];
      int rank = 0;
      for (int j = 0; j < a.K; ++j) {
        const int cj = cnt[j];
        rank += (cj > ck || (cj == ck && j < k)) ? 1 : 0;
      }
      a.korder[rank] = k;
    }
  }
}

__global__ __launch_bounds__(256) void gmm_bucket_scatter_kernel(GmmBucketArgs a) {
  extern __shared__ int hist[];  // [0, K): the block's next free slot inside each bucket | [K, 2K + 1): offsets | [.., 3K + 1): totals
  int* off = hist + a.K;
  bucket_offsets(a, off, off + a.K + 1);
  const int n_chunks = (a.n_end - a.n_begin + a.chunk - 1) / a.chunk;
  // the block's first slot inside every bucket: bucket offset + the counts of the blocks before it (binscan); the
  // walk over the chunks is the count kernel's, so the numbers match
  for (int k = threadIdx.x; k < a.K; k += 256) hist[k] = off[k] + a.blk_counts[(size_t)k * gridDim.x + blockIdx.x];
  __syncthreads();
  // place the elements (the order inside a bucket does not influence any result)
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int base = a.n_begin + c * a.chunk, size = bucket_chunk_size(a, c);
    if (a.seg_cnt && !a.ptab) {  // (uniform) candidate records of the arg-max screen: batched loads, same walk as the count kernel
      for (int i = threadIdx.x; i < size; i += 256 * BUCKET_UN) {
        int key[BUCKET_UN], patch[BUCKET_UN];
        record_keys<BUCKET_UN>(a, base, i, size, key, patch);
#pragma unroll
        for (int u = 0; u < BUCKET_UN; ++u)
          if (key[u] >= 0) {
            const int pos = atomicAdd(&hist[key[u]], 1);
            a.order[pos] = base + i + 256 * u;
            if (a.order_n) a.order_n[pos] = patch[u];
          }
      }
      continue;
    }
    for (int i = threadIdx.x; i < size; i += 256) {
      const int n = base + i;
      const int k = bucket_key(a, n);
      if (k >= 0) {
        const int pos = atomicAdd(&hist[k], 1);
        a.order[pos] = n;
        if (a.order_n) a.order_n[pos] = a.rec_n[n];
        if (a.ptab) {  // (the order of a patch's entries is whatever the atomics make it: the combine kernel sorts them)
          const int patch = a.rec_n[n];
          const int j = atomicAdd(a.pcount + patch, 1);
          if (j < a.ptab_rows)
            a.ptab[(size_t)patch * a.ptab_rows + j] = pos;
          else
            __hip_atomic_store(a.flag, a.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      } else if (k == -1 && a.gpatch) {  // filtered patch (patches/core.py:215-216): no gradient
        float4* row = reinterpret_cast<float4*>(a.gpatch + (size_t)(n - a.n_begin) * D);
        for (int q = 0; q < D / 4; ++q) row[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
}

void launch_bucket_sort(const GmmBucketArgs& bk, unsigned chunks, hipStream_t s) {
  const size_t hist_bytes = (size_t)bk.K * sizeof(int);
  gmm_bucket_count_kernel<<<chunks, 256, hist_bytes, s>>>(bk);
  launch_binscan(bk, bk.K, (int)chunks, s);
  gmm_bucket_scatter_kernel<<<chunks, 256, 3 * hist_bytes + sizeof(int), s>>>(bk);
}

}  // namespace jd
