// egg_orientation.h -- what api_egg_orientation.hip launches from egg_orientation.hip: the per-pixel median of a stack of uint8
// cut-outs, the nine sums of the two swap tests and the turn by 180 degrees of experiments_ovary_detect/run_egg_swap_orientation.py
// of the reference (compute_mean_image :92-98, condition_swap_correl :77-80, condition_swap_density :65-74,
// perform_orientation_swap :58-59).  Integers only.
#pragma once
#include "common.h"

namespace imsegm {

// the caps of include/imsegm_hip.h: the counters of the median are 16 bits wide, a pixel index and its mirror fit 32 bits
constexpr int EO_MAX_IMAGES = 65535, EO_MAX_CHANNELS = 4;
constexpr size_t EO_MAX_PIXELS = (size_t)1 << 30, EO_MAX_BYTES = ((size_t)1 << 31) - 1;
// the words of one image (IMSEGM_ORIENT_SUM_WORDS): a the channel, t template2, g = [a cnt > S]
enum { EO_A = 0, EO_MIN = 1, EO_MAX = 2, EO_P = 3, EO_PF = 4, EO_CNT = 5, EO_S = 6, EO_L = 7, EO_R = 8, EO_SUM_WORDS = 9 };
enum { EO_MODE_CC = 0, EO_MODE_DENSITY = 1 };

// planes[i hw + p] = stack[(i hw + p) C + channel]: the channel of all images as N planes of hw bytes
int launch_eo_extract(const uint8_t *stack, int N, size_t hw, int C, int channel, uint8_t *planes, hipStream_t st);
// template2[p] = s[(N - 1) / 2] + s[N / 2] of the N values planes[. hw + p] sorted: twice their median
int launch_eo_median(const uint8_t *planes, int N, size_t hw, uint16_t *template2, hipStream_t st);
// range[0], range[1] = the smallest and the largest word of template2 (range: two device words, set here)
int launch_eo_template_range(const uint16_t *template2, size_t hw, uint32_t *range, hipStream_t st);
// sums[i][EO_*] of image i (h x w bytes at planes + i h w) and flags[i] = the decision of `mode` from them and `range`
int launch_eo_sums(const uint8_t *planes, int N, int h, int w, const uint16_t *template2, const uint32_t *range, int mode, long long *sums,
                   uint8_t *flags, hipStream_t st);
// every image i of the interleaved stack with flags[i] set becomes img[::-1, ::-1, :], in place
int launch_eo_turn(uint8_t *stack, int N, size_t hw, int C, const uint8_t *flags, hipStream_t st);

}  // namespace imsegm
