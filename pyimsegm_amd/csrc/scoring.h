// scoring.h -- launchers of csrc/scoring.hip (contingency tables of annotation / segmentation pairs; the C ABI is in
// api_scoring.hip)
#pragma once
#include "../../include/imsegm_hip.h"
#include "common.h"

namespace imsegm {

constexpr int SCORE_MAX_LABELS = IMSEGM_SCORE_MAX_LABELS;
constexpr int SCORE_MAX_DROP = IMSEGM_SCORE_MAX_DROP;
constexpr int SCORE_THREADS = IMSEGM_SCORE_THREADS;
constexpr int SCORE_RUN = IMSEGM_SCORE_RUN;
constexpr int SCORE_CHUNK_STEPS = IMSEGM_SCORE_CHUNK_STEPS;
// pixels a workgroup owns: its 32-bit LDS counters cannot wrap, they are flushed once per workgroup
constexpr size_t SCORE_CHUNK_PIXELS = (size_t)SCORE_THREADS * SCORE_RUN * SCORE_CHUNK_STEPS;
constexpr int SCORE_WAVE_TABLE_LABELS = IMSEGM_SCORE_WAVE_TABLE_LABELS;
// bins of a pair's table in memory (row stride U, not MAX_LABELS) and of a workgroup's LDS
constexpr int SCORE_TABLE_BINS = SCORE_MAX_LABELS * SCORE_MAX_LABELS;
// slots of a label set (open addressing, 64-bit words: bit 32 marks a slot in use, the low word is the label)
constexpr int SCORE_SET_SLOTS = 2 * SCORE_MAX_LABELS;
static_assert((SCORE_SET_SLOTS & (SCORE_SET_SLOTS - 1)) == 0, "the probe sequence wraps with a mask");
static_assert((SCORE_THREADS / 64) * SCORE_WAVE_TABLE_LABELS * SCORE_WAVE_TABLE_LABELS <= SCORE_TABLE_BINS,
              "the per-wave tables share the LDS of the per-workgroup table");
static_assert(SCORE_CHUNK_PIXELS < ((size_t)1 << 32), "32-bit LDS counters");

// where pair i lies in the scratch (byte offsets from its base, 256-byte aligned) and how many elements it has
struct ScorePair {
    unsigned long long off_annot, off_segm, n;
};

// The device state of one call, all of it cleared by launch_score_pairs itself:
//   sets      n_pairs x SCORE_SET_SLOTS words, the label set of every pair
//   set_state n_pairs x 2 words: labels in the set, "too many" flag
//   status / n_labels n_pairs int32, labels n_pairs x SCORE_MAX_LABELS int32, tables n_pairs x SCORE_TABLE_BINS int64
struct ScoreState {
    unsigned long long *sets;
    unsigned int *set_state;
    int32_t *status, *n_labels, *labels;
    unsigned long long *tables;
};

// chunk_first: n_pairs + 1 words, the first chunk (workgroup) of every pair and, last, their total; drop: n_drop labels on the
// device.  Discovery, sort and count in one chain on `st`; `clear` / `clear_bytes` is the state's memory (one memset).
int launch_score_pairs(const unsigned char *base, const ScorePair *pairs, const unsigned int *chunk_first, int n_pairs,
                       unsigned int total_chunks, int dtype, const int32_t *drop, int n_drop, const ScoreState &state, void *clear,
                       size_t clear_bytes, hipStream_t st);

}  // namespace imsegm
