// scoring.hip -- contingency tables of (annotation, segmentation) pairs: the one object every score of imsegm/classification.py
// (:305-471) is a function of.  Three kernels in one chain over ALL pairs of a call:
//
//   k_score_discover  which labels does a pair hold?  Every workgroup owns SCORE_CHUNK_PIXELS consecutive pixels of one pair and keeps
//                     the labels of its pixels that survive dropping in an LDS set; it merges that set into the pair's set in memory
//                     once, at its end.
//   k_score_sort      one small workgroup per pair: the set's at most 64 labels in ascending order, their number and the status.
//   k_score_count     the same chunks again: the sorted labels in LDS, runs of equal (annot, segm) merged in registers, one LDS add
//                     per run, one 64-bit integer atomic per non-zero bin and workgroup at the end.
//
// Neither pixel pass issues a global atomic per pixel or per run; all atomics are integer adds / compare-and-swaps whose outcome
// does not depend on their order, so two calls give the same bytes.  HBM bound: 8 B per pixel and pass for int32, 2 B for uint8.
//
// The counting pass needs no drop list: a drop label is never in the pair's set (every pixel that carries it is dropped), and a
// pixel that stays has both its labels in the set, so "a label of the pixel is not in the set" IS "the pixel is dropped".
//
// LDS.  A workgroup's table is SCORE_TABLE_BINS = 64 x 64 32-bit counters, 16 KiB: eight workgroups (32 waves, all a CU holds) fit
// the 160 KiB of a gfx950 CU with room to spare, so LDS never limits occupancy.  While 4 U^2 <= 4096, that is U <=
// SCORE_WAVE_TABLE_LABELS = 32, each of the four waves counts into a U x U table of its own in that same array: lanes of different
// waves then never meet on a counter, which matters most where it is worst, on maps of two or three labels whose every run hits
// the same few bins.  Above 32 labels four tables no longer fit the 16 KiB and the waves share one; with that many bins they rarely
// meet.  A counter takes at most SCORE_CHUNK_PIXELS = 8192 pixels before it is flushed: it cannot wrap.
#include "scoring.h"

namespace imsegm {

namespace {

constexpr unsigned long long SET_USED = 1ull << 32;

__device__ inline unsigned set_hash(int32_t label) { return ((unsigned)label * 2654435761u) >> 25; }   // 7 bits: SCORE_SET_SLOTS
static_assert(SCORE_SET_SLOTS == 128, "set_hash yields 7 bits");

// the pair of workgroup `chunk`: the last one whose first chunk is not behind it (pairs without a chunk are stepped over)
__device__ inline int pair_of_chunk(const unsigned int *__restrict__ chunk_first, int n_pairs, unsigned int chunk)
{
    int lo = 0, hi = n_pairs;                         // chunk_first[lo] <= chunk < chunk_first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_first[mid] <= chunk) lo = mid;
        else hi = mid;
    }
    return lo;
}

// SCORE_RUN consecutive elements from `at` (a multiple of SCORE_RUN); the caller has checked at + SCORE_RUN <= n
__device__ inline void load_full(const int32_t *__restrict__ p, size_t at, int (&v)[SCORE_RUN])
{
    const int4 lo = *reinterpret_cast<const int4 *>(p + at), hi = *reinterpret_cast<const int4 *>(p + at + 4);
    v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

__device__ inline void load_full(const uint8_t *__restrict__ p, size_t at, int (&v)[SCORE_RUN])
{
    const uint2 w = *reinterpret_cast<const uint2 *>(p + at);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = (int)((w.x >> (8 * i)) & 255u);
        v[4 + i] = (int)((w.y >> (8 * i)) & 255u);
    }
}
static_assert(SCORE_RUN == 8, "load_full reads eight elements");

// the elements [at, at + SCORE_RUN) of both maps that lie below `end`; returns how many
template <typename T>
__device__ inline int load_pixels(const T *__restrict__ annot, const T *__restrict__ segm, size_t at, size_t end, int (&a)[SCORE_RUN],
                                  int (&s)[SCORE_RUN])
{
    if (at + SCORE_RUN <= end) {
        load_full(annot, at, a);
        load_full(segm, at, s);
        return SCORE_RUN;
    }
    const int m = (int)(end - at);
#pragma unroll
    for (int i = 0; i < SCORE_RUN; ++i) {
        a[i] = i < m ? (int)annot[at + i] : 0;
        s[i] = i < m ? (int)segm[at + i] : 0;
    }
    return m;
}

// adds `label` to a set of SCORE_SET_SLOTS words in LDS or in memory; *count and *over are the set's size and its "too many" flag.
// At most SCORE_SET_SLOTS probes: a set that is full raises the flag instead of spinning.
template <int SCOPE>
__device__ inline void set_insert(unsigned long long *set, unsigned int *count, unsigned int *over, int32_t label)
{
    const unsigned long long key = SET_USED | (unsigned long long)(unsigned)label;
    const unsigned h = set_hash(label);
    for (int probe = 0; probe < SCORE_SET_SLOTS; ++probe) {
        unsigned long long *slot = set + ((h + probe) & (SCORE_SET_SLOTS - 1));
        unsigned long long seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, SCOPE);
        if (seen == 0) {
            unsigned long long expected = 0;
            if (__hip_atomic_compare_exchange_strong(slot, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) {
                if (__hip_atomic_fetch_add(count, 1u, __ATOMIC_RELAXED, SCOPE) >= (unsigned)SCORE_MAX_LABELS)
                    __hip_atomic_store(over, 1u, __ATOMIC_RELAXED, SCOPE);
                return;
            }
            seen = expected;
        }
        if (seen == key) return;
    }
    __hip_atomic_store(over, 1u, __ATOMIC_RELAXED, SCOPE);
}

template <typename T>
__global__ void __launch_bounds__(SCORE_THREADS)
k_score_discover(const unsigned char *__restrict__ base, const ScorePair *__restrict__ pairs, const unsigned int *__restrict__ chunk_first,
                 int n_pairs, const int32_t *__restrict__ drop, int n_drop, unsigned long long *__restrict__ sets,
                 unsigned int *__restrict__ set_state)
{
    __shared__ unsigned long long s_set[SCORE_SET_SLOTS];
    __shared__ int32_t s_drop[SCORE_MAX_DROP];
    __shared__ unsigned int s_count, s_over;
    const int tid = threadIdx.x;
    const int pair = pair_of_chunk(chunk_first, n_pairs, blockIdx.x);
    const ScorePair pr = pairs[pair];
    if (tid < SCORE_SET_SLOTS) s_set[tid] = 0;
    if (tid < n_drop) s_drop[tid] = drop[tid];
    if (tid == 0) s_count = 0, s_over = 0;
    __syncthreads();
    const T *annot = reinterpret_cast<const T *>(base + pr.off_annot), *segm = reinterpret_cast<const T *>(base + pr.off_segm);
    const size_t begin = (size_t)(blockIdx.x - chunk_first[pair]) * SCORE_CHUNK_PIXELS;
    const size_t end = begin + SCORE_CHUNK_PIXELS < pr.n ? begin + SCORE_CHUNK_PIXELS : (size_t)pr.n;
    bool have = false;                                   // (pa, ps): the last pair of labels this lane has looked at
    int pa = 0, ps = 0;
    for (int step = 0; step < SCORE_CHUNK_STEPS; ++step) {
        const size_t at = begin + ((size_t)step * SCORE_THREADS + tid) * SCORE_RUN;
        if (at >= end) break;
        int a[SCORE_RUN], s[SCORE_RUN];
        const int m = load_pixels(annot, segm, at, end, a, s);
#pragma unroll
        for (int i = 0; i < SCORE_RUN; ++i) {
            if (i >= m || (have && a[i] == pa && s[i] == ps)) continue;
            have = true;
            pa = a[i];
            ps = s[i];
            bool dropped = false;
            for (int d = 0; d < n_drop; ++d) dropped |= s_drop[d] == pa || s_drop[d] == ps;
            if (dropped) continue;
            set_insert<__HIP_MEMORY_SCOPE_WORKGROUP>(s_set, &s_count, &s_over, pa);
            if (ps != pa) set_insert<__HIP_MEMORY_SCOPE_WORKGROUP>(s_set, &s_count, &s_over, ps);
        }
    }
    __syncthreads();
    unsigned int *state = set_state + 2 * (size_t)pair;
    if (s_over) {
        if (tid == 0) __hip_atomic_fetch_or(state + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (tid < SCORE_SET_SLOTS && s_set[tid])
        set_insert<__HIP_MEMORY_SCOPE_AGENT>(sets + (size_t)pair * SCORE_SET_SLOTS, state, state + 1, (int32_t)(unsigned)s_set[tid]);
}

__global__ void __launch_bounds__(SCORE_SET_SLOTS)
k_score_sort(const unsigned long long *__restrict__ sets, const unsigned int *__restrict__ set_state, int32_t *__restrict__ status,
             int32_t *__restrict__ n_labels, int32_t *__restrict__ labels)
{
    __shared__ int32_t s_vals[SCORE_SET_SLOTS];
    __shared__ unsigned int s_n;
    const int tid = threadIdx.x, pair = blockIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const unsigned long long word = sets[(size_t)pair * SCORE_SET_SLOTS + tid];
    if (word) s_vals[atomicAdd(&s_n, 1u)] = (int32_t)(unsigned)word;          // (at most SCORE_SET_SLOTS words: the index fits)
    __syncthreads();
    const int n = (int)s_n;
    if (set_state[2 * (size_t)pair + 1] || n > SCORE_MAX_LABELS) {
        if (tid == 0) {
            status[pair] = IMSEGM_SCORE_TOO_MANY_LABELS;
            n_labels[pair] = 0;                                                 // the counting pass skips the pair
        }
        return;
    }
    if (tid < n) {
        const int32_t mine = s_vals[tid];
        int rank = 0;                                                           // the labels are distinct: ranks are too
        for (int j = 0; j < n; ++j) rank += s_vals[j] < mine;
        labels[(size_t)pair * SCORE_MAX_LABELS + rank] = mine;
    }
    if (tid == 0) {
        status[pair] = IMSEGM_SCORE_OK;
        n_labels[pair] = n;
    }
}

// index of `label` in the ascending s_lab[0 .. U), -1 when it is not there
__device__ inline int label_index(const int32_t *s_lab, int U, int32_t label)
{
    int lo = 0, hi = U;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_lab[mid] < label) lo = mid + 1;
        else hi = mid;
    }
    return lo < U && s_lab[lo] == label ? lo : -1;
}

// `run` pixels of the pair (annot, segm) into the LDS table; a label outside the set marks dropped pixels
__device__ inline void count_run(unsigned int *tab, const int32_t *s_lab, int U, int32_t annot, int32_t segm, unsigned run)
{
    const int ia = label_index(s_lab, U, annot), ib = label_index(s_lab, U, segm);
    if (ia >= 0 && ib >= 0) atomicAdd(tab + ia * U + ib, run);
}

template <typename T>
__global__ void __launch_bounds__(SCORE_THREADS)
k_score_count(const unsigned char *__restrict__ base, const ScorePair *__restrict__ pairs, const unsigned int *__restrict__ chunk_first,
              int n_pairs, const int32_t *__restrict__ n_labels, const int32_t *__restrict__ labels, unsigned long long *__restrict__ tables)
{
    __shared__ int32_t s_lab[SCORE_MAX_LABELS];
    __shared__ unsigned int s_tab[SCORE_TABLE_BINS];
    const int tid = threadIdx.x;
    const int pair = pair_of_chunk(chunk_first, n_pairs, blockIdx.x);
    const int U = n_labels[pair];
    if (U < 1 || U > SCORE_MAX_LABELS) return;           // nothing survives dropping, or too many labels (uniform: no barrier is left behind)
    const int bins = U * U;
    const int copies = U <= SCORE_WAVE_TABLE_LABELS ? SCORE_THREADS / 64 : 1;
    for (int i = tid; i < copies * bins; i += SCORE_THREADS) s_tab[i] = 0;
    if (tid < U) s_lab[tid] = labels[(size_t)pair * SCORE_MAX_LABELS + tid];
    __syncthreads();
    unsigned int *tab = s_tab + (copies > 1 ? (tid >> 6) * bins : 0);
    const ScorePair pr = pairs[pair];
    const T *annot = reinterpret_cast<const T *>(base + pr.off_annot), *segm = reinterpret_cast<const T *>(base + pr.off_segm);
    const size_t begin = (size_t)(blockIdx.x - chunk_first[pair]) * SCORE_CHUNK_PIXELS;
    const size_t end = begin + SCORE_CHUNK_PIXELS < pr.n ? begin + SCORE_CHUNK_PIXELS : (size_t)pr.n;
    for (int step = 0; step < SCORE_CHUNK_STEPS; ++step) {
        const size_t at = begin + ((size_t)step * SCORE_THREADS + tid) * SCORE_RUN;
        if (at >= end) break;
        int a[SCORE_RUN], s[SCORE_RUN];
        const int m = load_pixels(annot, segm, at, end, a, s);
        int ca = a[0], cs = s[0];                        // the current run (m >= 1)
        unsigned run = 1;
#pragma unroll
        for (int i = 1; i < SCORE_RUN; ++i) {
            if (i >= m) continue;
            if (a[i] != ca || s[i] != cs) {
                count_run(tab, s_lab, U, ca, cs, run);
                ca = a[i];
                cs = s[i];
                run = 0;
            }
            run++;
        }
        count_run(tab, s_lab, U, ca, cs, run);
    }
    __syncthreads();
    unsigned long long *table = tables + (size_t)pair * SCORE_TABLE_BINS;
    for (int i = tid; i < bins; i += SCORE_THREADS) {
        unsigned long long sum = 0;
        for (int c = 0; c < copies; ++c) sum += s_tab[c * bins + i];
        if (sum) atomicAdd(table + i, sum);
    }
}

}  // namespace

int launch_score_pairs(const unsigned char *base, const ScorePair *pairs, const unsigned int *chunk_first, int n_pairs,
                       unsigned int total_chunks, int dtype, const int32_t *drop, int n_drop, const ScoreState &state, void *clear,
                       size_t clear_bytes, hipStream_t st)
{
    if (n_pairs < 1) return 0;
    HIP_TRY(hipMemsetAsync(clear, 0, clear_bytes, st));
    if (total_chunks) {
        if (dtype == IMSEGM_SCORE_U8)
            hipLaunchKernelGGL(k_score_discover<uint8_t>, total_chunks, SCORE_THREADS, 0, st, base, pairs, chunk_first, n_pairs, drop, n_drop,
                               state.sets, state.set_state);
        else
            hipLaunchKernelGGL(k_score_discover<int32_t>, total_chunks, SCORE_THREADS, 0, st, base, pairs, chunk_first, n_pairs, drop, n_drop,
                               state.sets, state.set_state);
    }
    hipLaunchKernelGGL(k_score_sort, n_pairs, SCORE_SET_SLOTS, 0, st, state.sets, state.set_state, state.status, state.n_labels, state.labels);
    if (total_chunks) {
        if (dtype == IMSEGM_SCORE_U8)
            hipLaunchKernelGGL(k_score_count<uint8_t>, total_chunks, SCORE_THREADS, 0, st, base, pairs, chunk_first, n_pairs, state.n_labels,
                               state.labels, state.tables);
        else
            hipLaunchKernelGGL(k_score_count<int32_t>, total_chunks, SCORE_THREADS, 0, st, base, pairs, chunk_first, n_pairs, state.n_labels,
                               state.labels, state.tables);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
