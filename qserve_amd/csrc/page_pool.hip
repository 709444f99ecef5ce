// page_pool.hip -- the device-side page allocator of the paged KV cache, for MI355X (gfx950): a free stack of page indices that is
// common to the K and V pools of every layer, and the two launches that move pages between the stack and the rows of the per-layer
// pointer tables without the host knowing a length.  DESIGN.md 10 ("Page pool and admission"); the rules are the header comment of
// qs_pages_reserve / qs_pages_release in include/qserve_amd.h, in exact integers.  This file holds SIX kernels.
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
//   pages_hold_kernel      (reference counts, qs_pages_hold) rows map pages that already have a holder: the prefix of `take` in row order,
//                every named id checked (range, refs != 0, hold_ids distinct through a mark per id in `scratch`), then the strided loop
//                writes page_ids and the tables and adds 1 to refs per naming entry; owned = take.
//   pages_unhold_kernel    (qs_pages_unhold) the list H of holds given up = the masked rows' pages, then drop_ids: per id its occurrences
//                (atomic add) and its first position in H (atomic max of len(H) - p) in `scratch`; the pages whose count reaches 0 are
//                pushed in the order of their first occurrence - a chunked scan over H of "first occurrence of a freed page" -, then
//                refs -= g, the rows end as after a release, and the scratch is zero again.
//   pages_fork_kernel      (qs_pages_fork, launch 1) destination rows branch off a source row: the whole pages below the source's last
//                written slot are mapped and counted as in a hold, one fresh page per destination is popped for the partly filled
//                tail - the prefix of `grow` (0 or 1) in row order, as the reserve serves -; a destination that cannot be served is
//                marked as the reserve marks a refused row.
//   pages_fork_copy_kernel (launch 2) a grid over (row, layer x K / V): the source's tail page, page_bytes bytes, into the fresh page
//                of every served destination - 16-byte vectors where the pages allow, bytes otherwise.
// The two uncounted entries use no atomics; the counted ones only integer add / max, whose result no arrival order changes.  No
// cross-workgroup traffic, vector stores only.  Every index is clamped before an address is formed from it.
//
// Each phase the five pool kernels share is written once, above them, and a kernel is its own steps between calls of these:
//   in_range -> free_count, owned_pages   a word read, flagged outside 0 .. n, clamped (steps 1: `count`, `owned`; hold's `take`)
//   chunk_scan -> scan_rows               the chunked wave scan (step 2; unhold's push order over H is the same primitive)
//   block_reduce -> block_max / _sum / _any
//   pop_count                             step 3 (reserve, fork)
//   fails                                 step 4: the one place that writes error[0]
//   page_address, table_row               what a table entry holds for a page id (N: the sink) and where a row's entries are - the
//                                         fill, the fork and the copy launch's check form no address of their own
//   for_each_slot                         step 5 around a kernel's per-slot action (reserve, release, hold, unhold)
//   masked_rows, clear_masked_rows        release's and unhold's steps 1 and 6;   refuse_row: reserve's and fork's refused row
// The helpers that hold a barrier say so; every thread of the workgroup calls them, under no divergent condition.  for_each_slot and
// the per-row helpers hold none.  The entries below share pool_args, which checks the common arguments and fills the record.
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
    const int* rows_mask;                            // [batch]            (release, unhold)
    int* refs;                                       // [N] or null        (holders per page; null: the uncounted reserve)
    int* scratch;                                    // [2 * N]            (hold, unhold: zero on entry, zero again on exit)
    const int* take;                                 // [batch]            (hold)
    const int* src;                                  // [batch, mb]        (hold)
    const int* extra_ids;                            // [num_extra] or null (hold: hold_ids; unhold: drop_ids)
    const int* src_rows;                             // [batch]            (fork: the row a destination branches off, or < 0)
    int num_extra;
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
__device__ __forceinline__ bool is_page(int id, int N) { return id >= 0 && id < N; }

// a word of the state that must lie in 0 .. n: flagged where it does not, and clamped
__device__ __forceinline__ int in_range(int v, int n, bool& bad) {
    bad = bad || v < 0 || v > n;
    return v < 0 ? 0 : v > n ? n : v;
}
__device__ __forceinline__ int free_count(const PoolArgs& a, bool& bad) { return in_range(a.count[0], a.N, bad); }
__device__ __forceinline__ int owned_pages(const PoolArgs& a, int b, bool& bad) { return in_range(a.owned[b], a.mb, bad); }

// what the table entry of a page holds, for (layer, K / V) w: the page's address in that pool; id = N is the sink
__device__ __forceinline__ long long page_address(const PoolArgs& a, int w, int id) { return a.layer_bases[w] + (long long)id * a.page_bytes; }
// the mb table entries of row b for (layer, K / V) w
__device__ __forceinline__ long long* table_row(const PoolArgs& a, int b, int w) {
    return reinterpret_cast<long long*>(a.layer_tables[w >> 1]) + ((size_t)b * 2 + (w & 1)) * a.mb;
}

// v folded over the workgroup by an associative, commutative op; every thread calls it (two barriers), every thread gets the result
template <class Op>
__device__ __forceinline__ int block_reduce(PoolShared& sh, int v, Op op) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh.wave[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh.wave[0];
#pragma unroll
    for (int w = 1; w < POOL_WAVES; ++w) v = op(v, sh.wave[w]);
    __syncthreads();
    return v;
}
__device__ __forceinline__ int block_max(PoolShared& sh, int v) {
    return block_reduce(sh, v, [](int x, int y) { return x > y ? x : y; });
}
__device__ __forceinline__ int block_sum(PoolShared& sh, int v) {
    return block_reduce(sh, v, [](int x, int y) { return x + y; });
}
__device__ __forceinline__ bool block_any(PoolShared& sh, bool flag) { return block_max(sh, flag ? 1 : 0) != 0; }

// step 4: whether any thread saw a broken invariant, and then error[0] = 1 - the caller writes nothing (more) and leaves.  Every thread
// calls it (block_any's barriers); the answer is workgroup-uniform.
__device__ __forceinline__ bool fails(const PoolArgs& a, PoolShared& sh, bool bad) {
    const bool any = block_any(sh, bad);
    if (any && threadIdx.x == 0) a.error[0] = 1;
    return any;
}

// One chunk of an inclusive prefix in thread order: a wave64 shuffle scan, the waves' totals through LDS, `carry` from the chunks before.
// out(carry + x_0 + .. + x_tid) runs between the two barriers; carry += the chunk's total.  Every thread calls it; ends behind a barrier
// (the next chunk, or a reduction, rewrites the waves' totals).
template <class Out>
__device__ __forceinline__ void chunk_scan(PoolShared& sh, int x, int& carry, Out out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
    out(x + before);
    carry += all;
    __syncthreads();
}

// S[b] = grow[0] + .. + grow[b] for every row -> the total.  Every thread of the workgroup calls it (barriers); ends behind a barrier.
__device__ __forceinline__ int scan_rows(PoolShared& sh, int batch) {
    int carry = 0;
    for (int c0 = 0; c0 < batch; c0 += POOL_THREADS) {                     // (workgroup-uniform)
        const int b = c0 + (int)threadIdx.x;
        chunk_scan(sh, b < batch ? sh.grow[b] : 0, carry, [&](int s) {
            if (b < batch) sh.S[b] = s;
        });
    }
    return carry;
}

// the row whose slots [S_b - grow_b, S_b) hold slot s: the first b with S_b > s (S is non-decreasing; s < S[batch - 1])
__device__ __forceinline__ int row_of_slot(const PoolShared& sh, int batch, int s) {
    int lo = 0, hi = batch - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sh.S[mid] > s) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// step 3 (reserve, fork): popped = the largest S_b <= cnt - S is monotone: a block maximum, <= cnt <= N -, and every id about to be
// popped is checked: in range, and without a holder where pages are counted.  Every thread calls it (block_max's barriers).
__device__ __forceinline__ int pop_count(const PoolArgs& a, PoolShared& sh, int cnt, bool& bad) {
    int mine = 0;
    for (int b = threadIdx.x; b < a.batch; b += POOL_THREADS) {
        const int S = sh.S[b];
        mine = S <= cnt && S > mine ? S : mine;
    }
    const int popped = block_max(sh, mine);
    for (int s = threadIdx.x; s < popped; s += POOL_THREADS) {
        const int id = a.free_list[clamp_index((long long)cnt - 1 - s, a.N)];
        bad = bad || !is_page(id, a.N);
        if (a.refs) bad = bad || a.refs[clamp_index(id, a.N)] != 0;         // (counted: a free page has no holder)
    }
    return popped;
}

// a row that asked for pages and gets none (reserve, fork)
__device__ __forceinline__ void refuse_row(const PoolArgs& a, int b) {
    a.starved[b] = 1;
    if (a.finished && a.finished[b] == 0) a.finished[b] = NO_PAGES;
}

// Step 5: the strided loop over (slot, layer, K / V) of the first `slots` slots of the prefix S.  The slot's row b by binary search, its
// place j among the row's slots; action(s, b, j, once) names the column and the page id the entry shall hold (N: the sink) and does,
// where `once` says so (one item per slot), what the kernel does once per slot; then the 8-byte store into that layer's table.  No
// barrier; the action clamps what it indexes with.
struct Slot {
    int col, id;
};
template <class Action>
__device__ __forceinline__ void for_each_slot(const PoolArgs& a, const PoolShared& sh, int slots, Action action) {
    const int lk = 2 * a.L;
    const long long items = (long long)slots * lk;
    for (long long it = threadIdx.x; it < items; it += POOL_THREADS) {
        const int s = (int)(it / lk), w = (int)(it - (long long)s * lk);
        const int b = row_of_slot(sh, a.batch, s);
        const Slot at = action(s, b, s - (sh.S[b] - sh.grow[b]), w == 0);
        table_row(a, b, w)[at.col] = page_address(a, w, at.id);
    }
}

// (release, unhold) step 1: grow = the pages of a masked row, 0 elsewhere; own = whether the row is masked; a masked row's ids checked
__device__ __forceinline__ void masked_rows(const PoolArgs& a, PoolShared& sh, bool& bad) {
    for (int b = threadIdx.x; b < a.batch; b += POOL_THREADS) {
        const int ownc = owned_pages(a, b, bad);
        const bool masked = a.rows_mask[b] != 0;
        sh.grow[b] = masked ? ownc : 0;
        sh.own[b] = masked ? 1 : 0;
        if (masked) {
            for (int j = 0; j < ownc; ++j) bad = bad || !is_page(a.page_ids[(size_t)b * a.mb + j], a.N);
        }
    }
}
// (release, unhold) step 6: the masked rows own nothing and are not starved
__device__ __forceinline__ void clear_masked_rows(const PoolArgs& a, const PoolShared& sh) {
    for (int b = threadIdx.x; b < a.batch; b += POOL_THREADS) {
        if (sh.own[b]) a.owned[b] = 0, a.starved[b] = 0;
    }
}

__global__ __launch_bounds__(POOL_THREADS) void pages_reserve_kernel(const PoolArgs a) {
    __shared__ PoolShared sh;
    const int tid = threadIdx.x;
    bool bad = false;
    const int cnt = free_count(a, bad);
    for (int b = tid; b < a.batch; b += POOL_THREADS) {
        const int ownc = owned_pages(a, b, bad);
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
    const int popped = pop_count(a, sh, cnt, bad);
    if (fails(a, sh, bad)) return;
    for_each_slot(a, sh, popped, [&](int s, int b, int j, bool once) {
        const int col = clamp_index((long long)sh.own[b] + j, a.mb);
        const int id = a.free_list[clamp_index((long long)cnt - 1 - s, a.N)];
        if (once) {
            a.page_ids[(size_t)b * a.mb + col] = id;
            if (a.refs) a.refs[id] = 1;                                     // (counted: the row is the page's one holder)
        }
        return Slot{col, id};
    });
    for (int b = tid; b < a.batch; b += POOL_THREADS) {
        const int g = sh.grow[b];
        if (g == 0) continue;
        if (sh.S[b] <= cnt) a.owned[b] = sh.own[b] + g; else refuse_row(a, b);
    }
    if (tid == 0) a.count[0] = cnt - popped;
}

__global__ __launch_bounds__(POOL_THREADS) void pages_release_kernel(const PoolArgs a) {
    __shared__ PoolShared sh;
    bool bad = false;
    const int cnt = free_count(a, bad);
    masked_rows(a, sh, bad);
    __syncthreads();
    const int total = scan_rows(sh, a.batch);
    bad = bad || (long long)cnt + total > a.N;
    if (fails(a, sh, bad)) return;
    for_each_slot(a, sh, total, [&](int s, int b, int j, bool once) {
        const int col = clamp_index(j, a.mb);
        if (once) {
            a.free_list[clamp_index((long long)cnt + s, a.N)] = a.page_ids[(size_t)b * a.mb + col];
            a.page_ids[(size_t)b * a.mb + col] = -1;
        }
        return Slot{col, a.N};
    });
    clear_masked_rows(a, sh);
    if (threadIdx.x == 0) a.count[0] = cnt + total;
}

// a scratch word that another thread of the workgroup changed by an atomic: read past the vector cache
__device__ __forceinline__ int scratch_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(POOL_THREADS) void pages_hold_kernel(const PoolArgs a) {
    __shared__ PoolShared sh;
    const int tid = threadIdx.x;
    bool bad = false;
    for (int b = tid; b < a.batch; b += POOL_THREADS) {
        const int tc = in_range(a.take[b], a.mb, bad);
        bad = bad || (tc > 0 && a.owned[b] != 0);
        sh.grow[b] = tc;
        for (int j = 0; j < tc; ++j) {
            const int id = a.src[(size_t)b * a.mb + j];
            bad = bad || !is_page(id, a.N) || a.refs[clamp_index(id, a.N)] == 0;
        }
    }
    __syncthreads();
    const int total = scan_rows(sh, a.batch);
    for (int k = tid; k < a.num_extra; k += POOL_THREADS) {
        const int id = a.extra_ids[k];
        bad = bad || !is_page(id, a.N) || a.refs[clamp_index(id, a.N)] == 0;
        if (is_page(id, a.N)) bad = bad || atomicAdd(&a.scratch[id], 1) != 0;   // (twice in hold_ids: whoever comes second sees it)
    }
    const bool failed = fails(a, sh, bad);                                  // (a barrier: every mark is set)
    for (int k = tid; k < a.num_extra; k += POOL_THREADS) {
        const int id = a.extra_ids[k];
        if (is_page(id, a.N)) a.scratch[id] = 0;
    }
    if (failed) return;
    for_each_slot(a, sh, total, [&](int s, int b, int j, bool once) {
        const int col = clamp_index(j, a.mb);
        const int id = clamp_index(a.src[(size_t)b * a.mb + col], a.N);
        if (once) {
            a.page_ids[(size_t)b * a.mb + col] = id;
            atomicAdd(&a.refs[id], 1);
        }
        return Slot{col, id};
    });
    for (int k = tid; k < a.num_extra; k += POOL_THREADS) atomicAdd(&a.refs[clamp_index(a.extra_ids[k], a.N)], 1);
    for (int b = tid; b < a.batch; b += POOL_THREADS) {
        if (sh.grow[b] > 0) a.owned[b] = sh.grow[b];
    }
}

// the id at position p of H (the masked rows' pages, then drop_ids), clamped; total = the rows' part
__device__ __forceinline__ int unhold_id(const PoolArgs& a, const PoolShared& sh, int total, int p) {
    if (p >= total) return clamp_index(a.extra_ids[p - total], a.N);
    const int b = row_of_slot(sh, a.batch, p);
    const int col = clamp_index((long long)p - (sh.S[b] - sh.grow[b]), a.mb);
    return clamp_index(a.page_ids[(size_t)b * a.mb + col], a.N);
}
// the scratch words of every id of H back to zero
__device__ __forceinline__ void unhold_clear(const PoolArgs& a, const PoolShared& sh, int total, int H) {
    for (int p = threadIdx.x; p < H; p += POOL_THREADS) {
        const int id = unhold_id(a, sh, total, p);
        a.scratch[id] = 0, a.scratch[a.N + id] = 0;
    }
}

__global__ __launch_bounds__(POOL_THREADS) void pages_unhold_kernel(const PoolArgs a) {
    __shared__ PoolShared sh;
    const int tid = threadIdx.x;
    int* occ = a.scratch;                                                   // [N]: g(id), the occurrences of id in H
    int* first = a.scratch + a.N;                                           // [N]: len(H) - the first position of id in H
    bool bad = false;
    const int cnt = free_count(a, bad);
    masked_rows(a, sh, bad);
    for (int k = tid; k < a.num_extra; k += POOL_THREADS) bad = bad || !is_page(a.extra_ids[k], a.N);
    __syncthreads();
    const int total = scan_rows(sh, a.batch);
    if (fails(a, sh, bad)) return;                                          // (the scratch is untouched)
    const int H = total + a.num_extra;
    // g(id) and the first occurrence of every id of H
    for (int p = tid; p < H; p += POOL_THREADS) {
        const int id = unhold_id(a, sh, total, p);
        atomicAdd(&occ[id], 1);
        atomicMax(&first[id], H - p);
    }
    __syncthreads();
    // more holds given up than there are; the pages that become free, counted
    int frees = 0;
    for (int p = tid; p < H; p += POOL_THREADS) {
        const int id = unhold_id(a, sh, total, p);
        const int g = scratch_load(&occ[id]), r = a.refs[id];
        bad = bad || g > r;
        frees += g == r && scratch_load(&first[id]) == H - p ? 1 : 0;
    }
    const int freed = block_sum(sh, frees);
    bad = bad || (long long)cnt + freed > a.N;
    if (fails(a, sh, bad)) {
        unhold_clear(a, sh, total, H);
        return;
    }
    // the freed pages onto the stack, in the order of their first occurrence in H: a scan over H in chunks
    int carry = 0;
    for (int p0 = 0; p0 < H; p0 += POOL_THREADS) {                          // (workgroup-uniform)
        const int p = p0 + tid;
        int id = 0, f = 0;
        if (p < H) {
            id = unhold_id(a, sh, total, p);
            f = scratch_load(&occ[id]) == a.refs[id] && scratch_load(&first[id]) == H - p ? 1 : 0;
        }
        chunk_scan(sh, f, carry, [&](int at) {
            if (f) a.free_list[clamp_index((long long)cnt + at - 1, a.N)] = id;
        });
    }
    // refs -= g, by the thread of the first occurrence (the others only read occ / first: barriers on both sides)
    for (int p = tid; p < H; p += POOL_THREADS) {
        const int id = unhold_id(a, sh, total, p);
        if (scratch_load(&first[id]) == H - p) a.refs[id] -= scratch_load(&occ[id]);
    }
    __syncthreads();
    unhold_clear(a, sh, total, H);
    __syncthreads();                                                        // (unhold_id reads page_ids: cleared only now)
    for_each_slot(a, sh, total, [&](int s, int b, int j, bool once) {
        const int col = clamp_index(j, a.mb);
        if (once) a.page_ids[(size_t)b * a.mb + col] = -1;
        return Slot{col, a.N};
    });
    clear_masked_rows(a, sh);
    if (tid == 0) a.count[0] = cnt + freed;
}

// what a fork asks of its source row, in the header's words: the page w and slot t of the last written position, and the pages to cover
struct ForkNeed {
    long long w, need;
    int t;
};
__device__ __forceinline__ ForkNeed fork_need(int length) {
    const long long len = length < 1 ? 1 : length;
    ForkNeed f;
    f.w = (len - 1) / 64, f.t = (int)((len - 1) % 64), f.need = f.w + (f.t > 0 ? 1 : 0);
    return f;
}
// whether destination d is served: its source covers the fork, and its fresh page, where it asks for one, is among the popped
__device__ __forceinline__ bool fork_served(const PoolShared& sh, int d, int cnt) {
    return sh.own[d] == 2 && (sh.grow[d] == 0 || sh.S[d] <= cnt);
}

// (qs_pages_fork, launch 1) destinations map the whole pages of their source and pop one fresh page for its tail.  sh.own holds a
// destination's case: 0 no destination, 1 refused by its source (the source does not cover the fork), 2 asks (grow = 0 or 1).
__global__ __launch_bounds__(POOL_THREADS) void pages_fork_kernel(const PoolArgs a) {
    __shared__ PoolShared sh;
    const int tid = threadIdx.x;
    bool bad = false;
    const int cnt = free_count(a, bad);
    for (int d = tid; d < a.batch; d += POOL_THREADS) {
        const int own = owned_pages(a, d, bad);
        const int s = a.src_rows[d];
        int state = 0, grow = 0;
        if (s >= 0) {
            const int sc = clamp_index(s, a.batch);
            bad = bad || s >= a.batch || s == d || a.src_rows[sc] >= 0 || own != 0;
            const ForkNeed f = fork_need(a.lengths[sc]);
            const int osc = owned_pages(a, sc, bad);                        // (flagged by the thread of row sc as well)
            const bool covered = f.need <= a.mb && osc >= f.need;
            const int named = f.need < osc ? (int)f.need : osc;              // <= mb
            for (int j = 0; j < named; ++j) {
                const int id = a.page_ids[(size_t)sc * a.mb + j];
                bad = bad || !is_page(id, a.N) || a.refs[clamp_index(id, a.N)] == 0;
            }
            state = covered ? 2 : 1;
            grow = covered && f.t > 0 ? 1 : 0;
        }
        sh.own[d] = state;
        sh.grow[d] = grow;
    }
    __syncthreads();
    scan_rows(sh, a.batch);
    const int popped = pop_count(a, sh, cnt, bad);
    if (fails(a, sh, bad)) return;
    // the fill, a strided loop over (destination, layer, K / V): the thread walks the row's columns (a source is no destination of
    // this launch: its page_ids are only read)
    const int lk = 2 * a.L;
    const long long items = (long long)a.batch * lk;
    for (long long it = tid; it < items; it += POOL_THREADS) {
        const int d = (int)(it / lk), w = (int)(it - (long long)d * lk);
        if (!fork_served(sh, d, cnt)) continue;
        const int sc = clamp_index(a.src_rows[d], a.batch);
        const ForkNeed f = fork_need(a.lengths[sc]);                        // (covered: need <= mb)
        long long* entries = table_row(a, d, w);
        for (int j = 0; j < (int)f.need; ++j) {
            const int col = clamp_index(j, a.mb);
            const bool fresh = j == (int)f.w;                               // (only with t > 0: need = w + 1)
            const int id = fresh ? a.free_list[clamp_index((long long)cnt - sh.S[d], a.N)]
                                 : clamp_index(a.page_ids[(size_t)sc * a.mb + col], a.N);
            if (w == 0) {
                a.page_ids[(size_t)d * a.mb + col] = id;
                if (fresh) a.refs[id] = 1; else atomicAdd(&a.refs[id], 1);
            }
            entries[col] = page_address(a, w, id);
        }
    }
    for (int d = tid; d < a.batch; d += POOL_THREADS) {
        if (sh.own[d] == 0) continue;
        if (fork_served(sh, d, cnt)) {
            const int sc = clamp_index(a.src_rows[d], a.batch);
            a.owned[d] = (int)fork_need(a.lengths[sc]).need;
        } else {
            refuse_row(a, d);
        }
    }
    if (tid == 0) a.count[0] = cnt - popped;
}

constexpr int COPY_THREADS = 256;
constexpr int COPY_SPLIT = 1;                        // workgroups per page (grid z): each copies one contiguous piece of it

// (qs_pages_fork, launch 2) workgroup (d, layer x K / V) copies the source's tail page to the fresh page of a served destination.
// Whether d is one is read from what launch 1 left: no index or address is formed from anything unchecked or unclamped, and the
// addresses are the two table entries launch 1 wrote - so the launch is safe behind an errored launch 1, and copies nothing then.
__global__ __launch_bounds__(COPY_THREADS) void pages_fork_copy_kernel(const PoolArgs a) {
    const int d = blockIdx.x, w = blockIdx.y;
    const int s = a.src_rows[d];
    if (s < 0 || s >= a.batch || s == d || a.error[0] != 0 || a.starved[d] != 0) return;
    const ForkNeed f = fork_need(a.lengths[s]);
    if (f.t == 0 || f.need > a.mb || a.owned[d] != (int)f.need || a.owned[s] < (int)f.need) return;
    const int col = clamp_index(f.w, a.mb);
    const int from = a.page_ids[(size_t)s * a.mb + col], to = a.page_ids[(size_t)d * a.mb + col];
    if (from == to || from < 0 || from >= a.N || to < 0 || to >= a.N) return;
    const long long src = table_row(a, s, w)[col], dst = table_row(a, d, w)[col];
    if (src != page_address(a, w, from) || dst != page_address(a, w, to)) return;
    const bool vectors = ((src | dst | a.page_bytes) & 15) == 0;
    const long long n = vectors ? a.page_bytes / 16 : a.page_bytes;          // this workgroup's piece: [lo, hi) of n vectors or bytes
    const long long piece = (n + gridDim.z - 1) / gridDim.z, lo = piece * blockIdx.z, hi = lo + piece < n ? lo + piece : n;
    if (vectors) {
        const uint4* p = reinterpret_cast<const uint4*>(src);
        uint4* q = reinterpret_cast<uint4*>(dst);
        for (long long i = lo + threadIdx.x; i < hi; i += COPY_THREADS) q[i] = p[i];
    } else {
        const unsigned char* p = reinterpret_cast<const unsigned char*>(src);
        unsigned char* q = reinterpret_cast<unsigned char*>(dst);
        for (long long i = lo + threadIdx.x; i < hi; i += COPY_THREADS) q[i] = p[i];
    }
}

// What every entry asks of the pool's state and geometry -> QS_OK and `a` filled with them, or QS_EINVAL with the message set.  rows:
// the entry's own per-row array, which must be there; opt1, opt2: further int32 arrays of its own that only have to be aligned.
int pool_args(PoolArgs& a, const char* what, int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved,
              int32_t* error, const int64_t* layer_tables, const int64_t* layer_bases, const void* rows, const void* opt1, const void* opt2,
              int batch, int max_blocks, int num_layers, int num_pages, int64_t page_bytes) {
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
    a = {};
    a.free_list = free_list, a.count = count, a.page_ids = page_ids, a.owned = owned, a.starved = starved, a.error = error;
    a.layer_tables = (const long long*)layer_tables, a.layer_bases = (const long long*)layer_bases;
    a.page_bytes = (long long)page_bytes, a.batch = batch, a.mb = max_blocks, a.L = num_layers, a.N = num_pages;
    return QS_OK;
}

// what the counted entries ask for on top of pool_args
int refs_arguments(const char* what, const int32_t* refs, const int32_t* scratch, bool with_scratch, const int32_t* ids, int num_ids,
                   int num_pages) {
    QS_REQUIRE(refs && (scratch || !with_scratch), "%s: null pointer (refs%s)", what, with_scratch ? ", scratch" : "");
    QS_REQUIRE(num_ids >= 0 && num_ids <= num_pages, "%s: %d ids (0 .. num_pages = %d)", what, num_ids, num_pages);
    QS_REQUIRE(ids || num_ids == 0, "%s: null id list of %d entries", what, num_ids);
    QS_REQUIRE((((uintptr_t)refs | (uintptr_t)scratch | (uintptr_t)ids) & 3) == 0, "%s: an int32 array is not 4-byte aligned", what);
    return QS_OK;
}

// one pool kernel, its one workgroup
int launch_pool(void (*kernel)(const PoolArgs), const PoolArgs& a, const char* what, qs_stream_t stream) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(POOL_THREADS), 0, (hipStream_t)stream, a);
    return qs_launch_status(what);
}

// qs_pages_reserve (counted = false: no refs) and qs_pages_reserve_refs
int reserve(const char* what, bool counted, int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved,
            int32_t* error, const int64_t* layer_tables, const int64_t* layer_bases, int32_t* refs, const int32_t* lengths,
            const int32_t* extra_rows, int32_t* finished, int batch, int max_blocks, int num_layers, int num_pages, int64_t page_bytes,
            int extra, qs_stream_t stream) {
    PoolArgs a;
    int rc = pool_args(a, what, free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, lengths, extra_rows, finished,
                       batch, max_blocks, num_layers, num_pages, page_bytes);
    if (rc != QS_OK) return rc;
    if (counted && (rc = refs_arguments(what, refs, nullptr, false, nullptr, 0, num_pages)) != QS_OK) return rc;
    QS_REQUIRE(extra >= 0, "%s: extra=%d (>= 0: the tokens the round is about to write)", what, extra);
    if (batch == 0) return QS_OK;
    a.lengths = lengths, a.extra_rows = extra_rows, a.finished = finished, a.extra = extra, a.refs = counted ? refs : nullptr;
    return launch_pool(pages_reserve_kernel, a, what, stream);
}

}  // namespace

extern "C" int qs_pages_reserve(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                                const int64_t* layer_tables, const int64_t* layer_bases, const int32_t* lengths, const int32_t* extra_rows,
                                int32_t* finished, int batch, int max_blocks, int num_layers, int num_pages, int64_t page_bytes, int extra,
                                qs_stream_t stream) {
    return reserve("pages_reserve", false, free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, nullptr, lengths,
                   extra_rows, finished, batch, max_blocks, num_layers, num_pages, page_bytes, extra, stream);
}

extern "C" int qs_pages_reserve_refs(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                                     const int64_t* layer_tables, const int64_t* layer_bases, int32_t* refs, const int32_t* lengths,
                                     const int32_t* extra_rows, int32_t* finished, int batch, int max_blocks, int num_layers, int num_pages,
                                     int64_t page_bytes, int extra, qs_stream_t stream) {
    return reserve("pages_reserve_refs", true, free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, refs, lengths,
                   extra_rows, finished, batch, max_blocks, num_layers, num_pages, page_bytes, extra, stream);
}

extern "C" int qs_pages_release(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                                const int64_t* layer_tables, const int64_t* layer_bases, const int32_t* rows_mask, int batch, int max_blocks,
                                int num_layers, int num_pages, int64_t page_bytes, qs_stream_t stream) {
    PoolArgs a;
    const int rc = pool_args(a, "pages_release", free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, rows_mask,
                             nullptr, nullptr, batch, max_blocks, num_layers, num_pages, page_bytes);
    if (rc != QS_OK) return rc;
    if (batch == 0) return QS_OK;
    a.rows_mask = rows_mask;
    return launch_pool(pages_release_kernel, a, "pages_release", stream);
}

extern "C" int qs_pages_hold(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                             const int64_t* layer_tables, const int64_t* layer_bases, int32_t* refs, int32_t* scratch, const int32_t* take,
                             const int32_t* src, const int32_t* hold_ids, int num_hold, int batch, int max_blocks, int num_layers,
                             int num_pages, int64_t page_bytes, qs_stream_t stream) {
    PoolArgs a;
    int rc = pool_args(a, "pages_hold", free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, take, src, nullptr,
                       batch, max_blocks, num_layers, num_pages, page_bytes);
    if (rc != QS_OK) return rc;
    QS_REQUIRE(src, "pages_hold: null pointer (src)");
    if ((rc = refs_arguments("pages_hold", refs, scratch, true, hold_ids, num_hold, num_pages)) != QS_OK) return rc;
    if (batch == 0 && num_hold == 0) return QS_OK;
    a.refs = refs, a.scratch = scratch, a.take = take, a.src = src, a.extra_ids = hold_ids, a.num_extra = num_hold;
    return launch_pool(pages_hold_kernel, a, "pages_hold", stream);
}

extern "C" int qs_pages_unhold(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                               const int64_t* layer_tables, const int64_t* layer_bases, int32_t* refs, int32_t* scratch,
                               const int32_t* rows_mask, const int32_t* drop_ids, int num_drop, int batch, int max_blocks, int num_layers,
                               int num_pages, int64_t page_bytes, qs_stream_t stream) {
    PoolArgs a;
    int rc = pool_args(a, "pages_unhold", free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, rows_mask, nullptr,
                       nullptr, batch, max_blocks, num_layers, num_pages, page_bytes);
    if (rc != QS_OK) return rc;
    if ((rc = refs_arguments("pages_unhold", refs, scratch, true, drop_ids, num_drop, num_pages)) != QS_OK) return rc;
    if (batch == 0 && num_drop == 0) return QS_OK;
    a.refs = refs, a.scratch = scratch, a.rows_mask = rows_mask, a.extra_ids = drop_ids, a.num_extra = num_drop;
    return launch_pool(pages_unhold_kernel, a, "pages_unhold", stream);
}

extern "C" int qs_pages_fork(int32_t* free_list, int32_t* count, int32_t* page_ids, int32_t* owned, int32_t* starved, int32_t* error,
                             const int64_t* layer_tables, const int64_t* layer_bases, int32_t* refs, const int32_t* src_rows,
                             const int32_t* lengths, int32_t* finished, int batch, int max_blocks, int num_layers, int num_pages,
                             int64_t page_bytes, qs_stream_t stream) {
    PoolArgs a;
    int rc = pool_args(a, "pages_fork", free_list, count, page_ids, owned, starved, error, layer_tables, layer_bases, src_rows, lengths,
                       finished, batch, max_blocks, num_layers, num_pages, page_bytes);
    if (rc != QS_OK) return rc;
    QS_REQUIRE(lengths, "pages_fork: null pointer (lengths)");
    if ((rc = refs_arguments("pages_fork", refs, nullptr, false, nullptr, 0, num_pages)) != QS_OK) return rc;
    if (batch == 0) return QS_OK;
    a.refs = refs, a.src_rows = src_rows, a.lengths = lengths, a.finished = finished;
    if ((rc = launch_pool(pages_fork_kernel, a, "pages_fork", stream)) != QS_OK) return rc;
    int split = COPY_SPLIT;
#ifdef QS_TIMING
    if (const char* e = getenv("QS_FORK_COPY_SPLIT")) split = atoi(e) < 1 ? 1 : atoi(e) > 64 ? 64 : atoi(e);   // (scripts/bench_fork.py)
#endif
    hipLaunchKernelGGL(pages_fork_copy_kernel, dim3(batch, 2 * num_layers, split), dim3(COPY_THREADS), 0, (hipStream_t)stream, a);
    return qs_launch_status("pages_fork (copy)");
}
