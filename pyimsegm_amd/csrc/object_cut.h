// object_cut.h -- what stands in front of the alpha-expansion when the graph is a 4-connected pixel grid (gco.cut_grid_graph) and
// when its unary costs are those of imsegm/region_growing.py object_segmentation_graphcut_pixels: the arcs of the grid in closed
// form, pyGCO's float -> integer conversion on the device, the object unary costs from a class map, a few centres and four tables.
// Kernels in object_cut.hip, C ABI in api_object_cut.hip.
#pragma once
#include "common.h"

namespace imsegm {

// edges of the H x W grid in pyGCO's order (all vertical edges row-major, then all horizontal ones) and its arcs
inline long grid_edges(int H, int W) { return (long)(H - 1) * W + (long)H * (W - 1); }

struct GridArcs {
    int32_t *edges;         // [E][2], a < b
    int32_t *arc_start;     // [K + 1]
    int32_t *arc_to;        // [2 E]
    int32_t *arc_rev;       // [2 E]
    int32_t *edge_arc;      // [E][2]
};
// the arrays the host loop of imsegm_cut_general_graph builds for that edge list, one thread per site
int launch_grid_arcs(int H, int W, GridArcs g, hipStream_t st);

// The four words of the conversion (device): bits of max |unary| and of max |weight| as unsigned 64-bit integers (a non-negative
// double orders like its bits), then -- written by launch_gc_convert -- the down-weight factor and max |int weight|.
enum { GC_RED_MU = 0, GC_RED_MW = 1, GC_RED_DWF = 2, GC_RED_WMAX = 3, GC_RED_WORDS = 4 };
// red[slot] = max(red[slot], max |x[i]|) (NaN is skipped as std::max skips it)
int launch_max_abs(const double *x, size_t n, unsigned long long *red, int slot, hipStream_t st);
// pyGCO: dwf = max(max|unary|, max|w| * max(pairwise)) + 1e-10 (the product only when pyGCO saw edges: have_edges); unary_i =
// (int32)((u / dwf) * 100000), w_i = (int32)((w / dwf) * 1000).  unary null: only the weights; w null: every weight is 1.
int launch_gc_convert(const double *unary, size_t n_unary, const double *w, int E, bool have_edges, double pairwise_max,
                      unsigned long long *red, int32_t *unary_i, int32_t *w_i, hipStream_t st);

// unary costs of object_segmentation_graphcut_pixels (imsegm/region_growing.py:202-242) from tables
struct ObjectUnary {
    const int32_t *segm;        // [H][W] class map; a negative class counts from the end of the tables as numpy indexes
    int H, W, n_centres;
    const int32_t *centres;     // [n_centres][4]: row, column the distance is taken from; row, column of the seed
    const double *a_bg, *a_fg, *s_bg;     // [n_labels]: -log(1 - p), -log(p), log(1 - p)
    int n_labels;
    const double *b;            // [n_dist]: log(1 - cdf(d) + 1e-9)
    int n_dist;
    double coef_shape;          // u = A - coef_shape * S when > 0, else u = A
    int seed_size;              // > 0: disc around the seed where segm > 0; else the seed pixel
};
constexpr size_t OBJECT_UNARY_LDS_MAX = 60 * 1024;
inline size_t object_unary_lds_bytes(int n_labels, int n_dist, int n_centres)
{
    return ((size_t)3 * n_labels + n_dist) * 8 + (size_t)n_centres * 16;
}
// pass 1: red[GC_RED_MU] = max |u| over all pixels and labels (seeds are 0)
int launch_object_unary_max(const ObjectUnary &o, unsigned long long *red, hipStream_t st);
// pass 2: unary_i[K][n_centres + 1] with the factor launch_gc_convert left in red[GC_RED_DWF]
int launch_object_unary_int(const ObjectUnary &o, const unsigned long long *red, int32_t *unary_i, hipStream_t st);

}  // namespace imsegm
