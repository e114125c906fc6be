// mixture_fit.h -- what the two families of the device mixture fit share (mixture_fit.hip: up to 16 features, a table row in
// registers; mixture_fit_wide.hip: 17 to 256 features, fp64 matrix tiles): the flags and caps of a restart's bookkeeping words and
// the host loop that enqueues iterations and looks at the `done` words.
#pragma once
#include "session.h"

namespace imsegm {

enum { FIT_FLAG_EMPTY = 1, FIT_FLAG_NOT_PD = 2 };
constexpr int FIT_MAX_C = 8, FIT_MAX_R = 16, FIT_ITERS_PER_LOOK = 8;

// run iterations until every restart is done: FIT_ITERS_PER_LOOK of them are enqueued, then the R `done` words are read
template <typename Step> int fit_iterate(const int *done_dev, int R, int max_iter, hipStream_t st, Step step)
{
    int done[FIT_MAX_R];
    for (int it = 0; it < max_iter;) {
        for (int k = 0; k < FIT_ITERS_PER_LOOK && it < max_iter; ++k, ++it)
            if (step()) return -1;
        HIP_TRY(hipMemcpyAsync(done, done_dev, (size_t)R * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bool all = true;
        for (int r = 0; r < R; ++r) all = all && done[r] != 0;
        if (all) break;
    }
    return 0;
}

}  // namespace imsegm
