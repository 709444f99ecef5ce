// page_pool.hip -- the device-side page allocator of the paged KV cache, for MI355X (gfx950): a free stack of page indices that is
// common to the K and V pools of every layer, and the two launches that move pages between the stack and the rows of the per-layer
// pointer tables without the host knowing a length.  DESIGN.md 10 ("Page pool and admission"); the rules are the header comment of
// qs_pages_reserve / qs_pages_release in include/qserve_amd.h, in exact integers.  This file holds TWO kernels.
//
//   pages_reserve_kernel   ONE workgroup of POOL_THREADS threads; rows are walked in chunks of POOL_THREADS (batch <= MAX_ROWS).
//                1. per row: owned (checked, clamped), need, grow -> LDS;
//                2. the inclusive prefix S of grow in row order: a wave64 shuffle scan per chunk, the waves' totals through LDS, a carry
//                   from chunk to chunk;
//                3. popped = the largest S_b <= count (S is monotone: a block maximum); the ids about to be popped are checked;
//                4. any broken invariant: error[0] = 1, nothing else is written, the launch ends;
//                5. the fill, a strided loop over (popped slot, layer, K / V): the slot's row by binary search over S in LDS, its page id
//                   from the stack, one 8-byte store into that layer's table (and, once per slot, page_ids);
//                6. per row: owned += grow, or starved / finished; thread 0: count -= popped.
//   pages_release_kernel   the same shape: prefix of `owned` over the masked rows, ids checked, then the strided loop pushes the ids,
//                clears page_ids and points the table entries at the sink; owned = starved = 0; count += the total.
// No atomics, no cross-workgroup traffic, vector stores only.  Every index is clamped before an address is formed from it.
#include "common.h"

namespace {

constexpr int POOL_THREADS = 256;                    // the one workgroup (4 waves): the stride of every row loop
constexpr int POOL_WAVES = POOL_THREADS / 64;
constexpr int MAX_ROWS = 1024;                       // rows of a batch (their prefix lives in LDS)
constexpr int NO_PAGES = 3;                          // `finished`: refused pages (qserve_amd.stopping.NO_PAGES)

struct PoolArgs {
    int* free_list;                                  // [N]
    int* count;                                      // [1]
    int* page_ids;                                   // [batch, mb]
    int* owned;                                      // [batch]
    int* starved;                                    // [batch]
    int* error;                                      // [1]
    const long long* layer_tables;                   // [L]: addresses of int64 [batch, 2, mb]
    const long long* layer_bases;                    // [L, 2]: K / V pool base addresses
    const int* lengths;                              // [batch]            (reserve)
    const int* extra_rows;                           // [batch] or null    (reserve)
    int* finished;                                   // [batch] or null    (reserve)
    const int* rows_mask;                            // [batch]            (release)
    long long page_bytes;
    int batch, mb, L, N, extra;
};

struct PoolShared {
    int S[MAX_ROWS];                                 // inclusive prefix, in row order
    int grow[MAX_ROWS];                              // what the prefix sums: a row's new pages (reserve), its pages (release)
    int own[MAX_ROWS];                               // owned on entry, clamped to 0 .. mb
    int wave[POOL_WAVES];
};

__device__ __forceinline__ int clamp_index(long long v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : (int)v; }

// S[b] = grow[0] + .. + grow[b] for every row -> the total.  Every thread of the workgroup calls it (barriers); ends behind a barrier.
__device__ __forceinline__ int scan_rows(PoolShared& sh, int batch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int c0 = 0; c0 < batch; c0 += POOL_THREADS) {                     // (workgroup-uniform)
        const int b = c0 + (int)threadIdx.x;
        int x = b < batch ? sh.grow[b] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(x, o, 64);
            if (lane >= o) x += t;
        }
        if (lane == 63) sh.wave[wave] = x;
        __syncthreads();
        int before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < POOL_WAVES; ++w) {
            const int t = sh.wave[w];
            before += w < wave ? t : 0;
            all += t;
        }
        if (b < batch) sh.S[b] = x + before;
        carry += all;
        __syncthreads();                                                    // (the next chunk rewrites the waves' totals)
    }
    return carry;
}

// max of v over the workgroup / whether any thread's flag is set; every thread calls them, every thread gets the result
__device__ __forceinline__ int block_max(PoolShared& sh, int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    if ((threadIdx.x & 63) == 0) sh.wave[threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < POOL_WAVES; ++w) v = sh.wave[w] > v ? sh.wave[w] : v;
    __syncthreads();
    return v;
}
__device__ __forceinline__ bool block_any(PoolShared& sh, bool flag) { return block_max(sh, flag ? 1 : 0) != 0; }

// the row whose slots [S_b - grow_b, S_b) hold slot s: the first b with S_b > s (S is non-decreasing; s < S[batch - 1])
__device__ __forceinline__ int row_of_slot(const PoolShared& sh, int batch, int s) {
    int lo = 0, hi = batch - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sh.S[mid] > s) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(POOL_THREADS) void pages_reserve_kernel(const PoolArgs a) {
    __shared__ PoolShared sh;
    const int tid = threadIdx.x;
    const int count = a.count[0];
    bool bad = count < 0 || count > a.N;
    const int cnt = count < 0 ? 0 : count > a.N ? a.N : count;
    for (int b = tid; b < a.batch; b += POOL_THREADS) {
        const int own = a.owned[b];
        bad = bad || own < 0 || own > a.mb;
        const int ownc = own < 0 ? 0 : own > a.mb ? a.mb : own;
        long long len = a.lengths[b], e = a.extra_rows ? a.extra_rows[b] : a.extra;
        len = len < 1 ? 1 : len;
        e = e < 0 ? 0 : e;
        long long need = (len - 1 + e + 63) / 64;
        need = need > a.mb ? a.mb : need;
        const bool fin = a.finished && a.finished[b] != 0;
        sh.grow[b] = fin || need <= ownc ? 0 : (int)need - ownc;
        sh.own[b] = ownc;
    }
    __syncthreads();
    scan_rows(sh, a.batch);
    int mine = 0;
    for (int b = tid; b < a.batch; b += POOL_THREADS) {
        const int S = sh.S[b];
        mine = S <= cnt && S > mine ? S : mine;
    }
    const int popped = block_max(sh, mine);                                 // <= cnt <= N
    for (int s = tid; s < popped; s += POOL_THREADS) {
        const int id = a.free_list[clamp_index((long long)cnt - 1 - s, a.N)];
        bad = bad || id < 0 || id >= a.N;
    }
    if (block_any(sh, bad)) {                                               // (workgroup-uniform)
        if (tid == 0) a.error[0] = 1;
        return;
    }
    const int lk = 2 * a.L;
    const long long items = (long long)popped * lk;
    for (long long it = tid; it < items; it += POOL_THREADS) {
        const int s = (int)(it / lk), w = (int)(it - (long long)s * lk);
        const int b = row_of_slot(sh, a.batch, s);
        const int j = s - (sh.S[b] - sh.grow[b]);
        const int col = clamp_index((long long)sh.own[b] + j, a.mb);
        const int id = a.free_list[clamp_index((long long)cnt - 1 - s, a.N)];
        if (w == 0) a.page_ids[(size_t)b * a.mb + col] = id;
        long long* table = reinterpret_cast<long long*>(a.layer_tables[w >> 1]);
        table[((size_t)b * 2 + (w & 1)) * a.mb + col] = a.layer_bases[w] + (long long)id * a.page_bytes;
    }
    for (int b = tid; b < a.batch; b += POOL_THREADS) {
        const int g = sh.grow[b];
        if (g == 0) continue;
        if (sh.S[b] <= cnt) {
            a.owned[b] = sh.own[b] + g;
        } else {
            a.starved[b] = 1;
            if (a.finished && a.finished[b] == 0) a.finished[b] = NO_PAGES;
        }
    }
    if (tid == 0) a.count[0] = cnt - popped;
}

__global__ __launch_bounds__(POOL_THREADS) void pages_release_kernel(const PoolArgs a) {
    __shared__ PoolShared sh;
    const int tid = threadIdx.x;
    const int count = a.count[0];
    bool bad = count < 0 || count > a.N;
    const int cnt = count < 0 ? 0 : count > a.N ? a.N : count;
    for (int b = tid; b < a.batch; b += POOL_THREADS) {
        const int own = a.owned[b];
        bad = bad || own < 0 || own > a.mb;
        const int ownc = own < 0 ? 0 : own > a.mb ? a.mb : own;
        const bool masked = a.rows_mask[b] != 0;
        sh.grow[b] = masked ? ownc : 0;
        sh.own[b] = masked ? 1 : 0;                                         // (release: whether the row is masked)
        if (masked) {
            for (int j = 0; j < ownc; ++j) {
                const int id = a.page_ids[(size_t)b * a.mb + j];
                bad = bad || id < 0 || id >= a.N;
            }
        }
    }
    __syncthreads();
    const int total = scan_rows(sh, a.batch);
    bad = bad || (long long)cnt + total > a.N;
    if (block_any(sh, bad)) {                                               // (workgroup-uniform)
        if (tid == 0) a.error[0] = 1;
        return;
    }
    const int lk = 2 * a.L;
    const long long items = (long long)total * lk;
    for (long long it = tid; it < items; it += POOL_THREADS) {
        const int s = (int)(it / lk), w = (int)(it - (long long)s * lk);
        const int b = row_of_slot(sh, a.batch, s);
        const int col = clamp_index((long long)s - (sh.S[b] - sh.grow[b]), a.mb);
        if (w == 0) {
            a.free_list[clamp_index((long long)cnt + s, a.N)] = a.page_ids[(size_t)b * a.mb + col];
            a.page_ids[(size_t)b * a.mb + col] = -1;
        }
        long long* table = reinterpret_cast<long long*>(a.layer_tables[w >> 1]);
        table[((size_t)b * 2 + (w & 1)) * a.mb + col] = a.layer_bases[w] + (long long)a.N * a.page_bytes;   // the sink
    }
    for (int b = tid; b < a.batch; b += POOL_THREADS) {
        if (sh.own[b]) a.owned[b] = 0, a.starved[b] = 0;
    }
    if (tid == 0) a.count[0] = cnt + total;
}

// what both entries ask for -> QS_OK, or QS_EINVAL with the message set
int pool_arguments(const char* what, const int32_t* free_list, const int32_t* count, const int32_t* page_ids, const int32_t* owned,
                   const int32_t* starved, const int32_t* error, const int64_t* layer_tables, const int64_t* layer_bases, const void* rows,
                   const void* opt1, const void* opt2, int batch, int max_blocks, int num_layers, int num_pages, int64_t page_bytes) {
    QS_REQUIRE(free_list && count && page_ids && owned && starved && error && layer_tables && layer_bases && rows, "%s: null pointer", what);
    QS_REQUIRE(num_pages >= 1, "%s: num_pages=%d (a pool has at least one page besides the sink)", what, num_pages);
    QS_REQUIRE(max_blocks >= 1 && num_layers >= 1, "%s: max_blocks=%d, num_layers=%d (>= 1)", what, max_blocks, num_layers);
    QS_REQUIRE(page_bytes >= 1 && num_pages < (1 << 30) / num_layers, "%s: page_bytes=%lld (>= 1), num_pages * num_layers=%lld (< 2^30)", what,
               (long long)page_bytes, (long long)num_pages * num_layers);
    QS_REQUIRE(batch >= 0 && batch <= MAX_ROWS, "%s: batch=%d (0 .. %d: one workgroup scans the rows)", what, batch, MAX_ROWS);
    QS_REQUIRE((long long)batch * max_blocks < (1ll << 31) / (2 * num_layers), "%s: batch * max_blocks * 2 * num_layers=%lld (< 2^31)", what,
               (long long)batch * max_blocks * 2 * num_layers);
    const uintptr_t words = (uintptr_t)free_list | (uintptr_t)count | (uintptr_t)page_ids | (uintptr_t)owned | (uintptr_t)starved |
                            (uintptr_t)error | (uintptr_t)rows | (uintptr_t)opt1 | (uintptr_t)opt2;
    QS_REQUIRE((words & 3) == 0, "%s: an int32 array is not 4-byte aligned", what);
    QS_REQUIRE((((uintptr_t)layer_tables | (uintptr_t)layer_bases) & 7) == 0, "%s: layer_tables and layer_bases must be 8-byte aligned", what);
    return QS_OK;
}

PoolArgs pool_args(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                   const int64_t* layer_tables, const int64_t* layer_bases, int batch, int max_blocks, int num_layers, int num_pages,
                   int64_t page_bytes) {
    PoolArgs a = {};
    a.free_list = free_list, a.count = count, a.page_ids = page_ids, a.owned = owned, a.starved = starved, a.error = error;
    a.layer_tables = (const long long*)layer_tables, a.layer_bases = (const long long*)layer_bases;
    a.page_bytes = (long long)page_bytes, a.batch = batch, a.mb = max_blocks, a.L = num_layers, a.N = num_pages;
    return a;
}

}  // namespace

extern "C" int qs_pages_reserve(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                                const int64_t* layer_tables, const int64_t* layer_bases, const int32_t* lengths, const int32_t* extra_rows,
                                int32_t* finished, int batch, int max_blocks, int num_layers, int num_pages, int64_t page_bytes, int extra,
                                qs_stream_t stream) {
    const int rc = pool_arguments("pages_reserve", free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, lengths,
                                  extra_rows, finished, batch, max_blocks, num_layers, num_pages, page_bytes);
    if (rc != QS_OK) return rc;
    QS_REQUIRE(extra >= 0, "pages_reserve: extra=%d (>= 0: the tokens the round is about to write)", extra);
    if (batch == 0) return QS_OK;
    PoolArgs a = pool_args(free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, batch, max_blocks, num_layers,
                           num_pages, page_bytes);
    a.lengths = lengths, a.extra_rows = extra_rows, a.finished = finished, a.extra = extra;
    hipLaunchKernelGGL(pages_reserve_kernel, dim3(1), dim3(POOL_THREADS), 0, (hipStream_t)stream, a);
    return qs_launch_status("pages_reserve");
}

extern "C" int qs_pages_release(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                                const int64_t* layer_tables, const int64_t* layer_bases, const int32_t* rows_mask, int batch, int max_blocks,
                                int num_layers, int num_pages, int64_t page_bytes, qs_stream_t stream) {
    const int rc = pool_arguments("pages_release", free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, rows_mask,
                                  nullptr, nullptr, batch, max_blocks, num_layers, num_pages, page_bytes);
    if (rc != QS_OK) return rc;
    if (batch == 0) return QS_OK;
    PoolArgs a = pool_args(free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, batch, max_blocks, num_layers,
                           num_pages, page_bytes);
    a.rows_mask = rows_mask;
    hipLaunchKernelGGL(pages_release_kernel, dim3(1), dim3(POOL_THREADS), 0, (hipStream_t)stream, a);
    return qs_launch_status("pages_release");
}
