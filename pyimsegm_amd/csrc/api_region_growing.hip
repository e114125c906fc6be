// api_region_growing.hip -- C ABI of the resident state of one region growing (imsegm/region_growing.py
// region_growing_shape_slic_greedy :1155, region_growing_shape_slic_graphcut :1482) on top of a label session: the label map goes
// up once (imsegm_image2d_set_labels), every iteration sends K labels and reads back its candidates.  Arguments are checked before
// the device is touched -- every index the kernels form comes from a value checked here; the kernels are in region_growing.hip.
#include "region_growing.h"
#include "session.h"

#include <cmath>
#include <vector>

struct imsegm_rg {
    imsegm_image2d *im = nullptr;       // read by every call except imsegm_rg_close
    int device = 0;                     // of im's context: close frees the buffers even after the session has gone
    RgView v;
    DevBuf state, job;
};

namespace {

int rg_bind(imsegm_rg *rg)
{
    if (!rg || !rg->im) {
        set_error("null region growing state");
        return -1;
    }
    return bind(rg->im->ctx);
}

// a new label vector (null: the resident one stays); labels index the columns of the cost tables
int rg_put_labels(imsegm_rg *rg, const int32_t *labels)
{
    if (!labels) return 0;
    for (int s = 0; s < rg->v.K; ++s)
        if (labels[s] < 0 || labels[s] > rg->v.n_obj) {
            set_error("region growing: label " + std::to_string(labels[s]) + " of superpixel " + std::to_string(s) + " is outside [0, objects]");
            return -1;
        }
    HIP_TRY(hipMemcpyAsync(rg->v.labels, labels, (size_t)rg->v.K * 4, hipMemcpyHostToDevice, rg->im->ctx->stream));
    return 0;
}

int rg_coefs(const double *coefs, RgCoefs &c)
{
    if (!coefs) {
        set_error("region growing: null coefficients");
        return -1;
    }
    c.data = coefs[0];
    c.shape = coefs[1];
    c.pairwise = coefs[2];
    c.pen_bg = coefs[3];
    c.pen_fg = coefs[4];
    return 0;
}

}  // namespace

extern "C" {

int imsegm_rg_open(imsegm_image2d *im, const int32_t *edges, int n_edges, int n_objects, imsegm_rg **rg_out)
{
    if (!im || !rg_out || bind(im->ctx)) return -1;
    if (wrong_kind(im, false)) return -1;
    if (!im->have_labels) {
        set_error("rg_open needs a label map");
        return -1;
    }
    const int K = im->n_labels;
    if (n_objects < 1 || n_edges < 0 || (n_edges > 0 && !edges) || (double)n_objects * (double)K > (double)(1 << 30)) {
        set_error("rg_open: at least one object, an edge list and at most 2^30 (object, superpixel) pairs are required");
        return -1;
    }
    std::vector<int32_t> off((size_t)K + 1, 0), nb((size_t)2 * n_edges + 1, 0);
    for (int e = 0; e < n_edges; ++e) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        if (a < 0 || a >= K || b < 0 || b >= K || a == b) {
            set_error("rg_open: edge " + std::to_string(e) + " does not join two different labels of the map");
            return -1;
        }
        off[(size_t)a + 1] += 1;
        off[(size_t)b + 1] += 1;
    }
    for (int k = 0; k < K; ++k) off[(size_t)k + 1] += off[k];
    {
        // the neighbour lists in the order get_neighboring_segments builds them (edge by edge, both ends)
        std::vector<int32_t> fill(off.begin(), off.end() - 1);
        for (int e = 0; e < n_edges; ++e) {
            const int a = edges[2 * e], b = edges[2 * e + 1];
            nb[fill[a]++] = b;
            nb[fill[b]++] = a;
        }
    }
    // pixel counts, coordinate sums and centres of the map: the session's graph pass leaves them at the head of its buffer
    int found = 0;
    if (imsegm_image2d_graph(im, nullptr, std::max(n_edges, 64), &found, nullptr, nullptr)) return -1;
    if (found != n_edges) {
        set_error("rg_open: the label map has " + std::to_string(found) + " edges, the list " + std::to_string(n_edges));
        return -1;
    }
    hipStream_t st = im->ctx->stream;
    const long long *cacc = im->graph.as<long long>();
    const double *centres = reinterpret_cast<const double *>(im->graph.as<unsigned char>() + (size_t)K * 3 * 8);

    imsegm_rg *rg = new imsegm_rg();
    rg->im = im;
    rg->device = im->ctx->device;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t pairs = (size_t)n_objects * K, table = (size_t)K * (n_objects + 1) * 8;
    const size_t o_points = take((size_t)K * 8), o_sums = take((size_t)K * 24), o_edges = take((size_t)n_edges * 8 + 8);
    const size_t o_off = take(((size_t)K + 1) * 4), o_nb = take(nb.size() * 4), o_data = take(table), o_shape = take(table);
    const size_t o_labels = take((size_t)K * 4), o_flags = take(pairs), o_slots = take((pairs + 1) * 4);
    const size_t o_cobj = take(pairs * 4), o_csp = take(pairs * 4), o_change = take(pairs * 8), o_crit = take(8);
    if (rg->state.ensure(at)) {
        delete rg;
        return -1;
    }
    unsigned char *dev = rg->state.as<unsigned char>();
    RgView &v = rg->v;
    v.K = K;
    v.n_obj = n_objects;
    v.E = n_edges;
    v.H = im->H;
    v.W = im->W;
    v.slic = im->labels.as<int32_t>();
    v.points = reinterpret_cast<int32_t *>(dev + o_points);
    v.sums = reinterpret_cast<long long *>(dev + o_sums);
    v.edges = reinterpret_cast<const int32_t *>(dev + o_edges);
    v.nb_off = reinterpret_cast<const int32_t *>(dev + o_off);
    v.nb = reinterpret_cast<const int32_t *>(dev + o_nb);
    v.lut_data = reinterpret_cast<double *>(dev + o_data);
    v.lut_shape = reinterpret_cast<double *>(dev + o_shape);
    v.labels = reinterpret_cast<int32_t *>(dev + o_labels);
    v.flags = dev + o_flags;
    v.slots = reinterpret_cast<int32_t *>(dev + o_slots);
    v.cand_obj = reinterpret_cast<int32_t *>(dev + o_cobj);
    v.cand_sp = reinterpret_cast<int32_t *>(dev + o_csp);
    v.cand_change = reinterpret_cast<double *>(dev + o_change);
    v.crit = reinterpret_cast<double *>(dev + o_crit);
    bool ok = hip_ok(hipMemsetAsync(dev, 0, at, st), "hipMemsetAsync", __FILE__, __LINE__) &&
              hip_ok(hipMemcpyAsync(v.sums, cacc, (size_t)K * 24, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync", __FILE__, __LINE__) &&
              launch_rg_points(centres, K, v.points, st) == 0 &&
              hip_ok(hipMemcpyAsync(dev + o_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync", __FILE__, __LINE__) &&
              hip_ok(hipMemcpyAsync(dev + o_nb, nb.data(), nb.size() * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync", __FILE__, __LINE__);
    if (ok && n_edges > 0)
        ok = hip_ok(hipMemcpyAsync(dev + o_edges, edges, (size_t)n_edges * 8, hipMemcpyHostToDevice, st), "hipMemcpyAsync", __FILE__, __LINE__);
    ok = ok && hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize", __FILE__, __LINE__);
    if (!ok) {
        rg->state.release();
        delete rg;
        return -1;
    }
    *rg_out = rg;
    return 0;
}

void imsegm_rg_close(imsegm_rg *rg)
{
    if (!rg) return;
    (void)hipSetDevice(rg->device);
    rg->state.release();
    rg->job.release();
    delete rg;
}

int imsegm_rg_get(imsegm_rg *rg, int what, void *out)
{
    if (rg_bind(rg)) return -1;
    const RgView &v = rg->v;
    const void *src = nullptr;
    size_t bytes = 0;
    if (what == 0) {
        src = v.sums;
        bytes = (size_t)v.K * 24;
    } else if (what == 1) {
        src = v.points;
        bytes = (size_t)v.K * 8;
    } else if (what == 2) {
        src = v.lut_shape;
        bytes = (size_t)v.K * (v.n_obj + 1) * 8;
    }
    if (!src || !out) {
        set_error("rg_get: 0 (sums), 1 (points) or 2 (shape costs) into a host array");
        return -1;
    }
    hipStream_t st = rg->im->ctx->stream;
    HIP_TRY(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_rg_set_costs(imsegm_rg *rg, const double *lut_data, const double *lut_shape)
{
    if (rg_bind(rg)) return -1;
    const size_t bytes = (size_t)rg->v.K * (rg->v.n_obj + 1) * 8;
    hipStream_t st = rg->im->ctx->stream;
    if (lut_data) HIP_TRY(hipMemcpyAsync(rg->v.lut_data, lut_data, bytes, hipMemcpyHostToDevice, st));
    if (lut_shape) HIP_TRY(hipMemcpyAsync(rg->v.lut_shape, lut_shape, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_rg_shape_costs(imsegm_rg *rg, int n_selected, const int32_t *objects, const double *centres, const double *shifts,
                          const int32_t *dims, const double *tables, double *proba_out)
{
    if (rg_bind(rg)) return -1;
    if (n_selected == 0) return 0;
    if (n_selected < 0 || !objects || !centres || !shifts || !dims || !tables) {
        set_error("rg_shape_costs: null array");
        return -1;
    }
    const RgView &v = rg->v;
    std::vector<long long> offsets((size_t)n_selected);
    long long total = 0;
    for (int j = 0; j < n_selected; ++j) {
        if (objects[j] < 0 || objects[j] >= v.n_obj) {
            set_error("rg_shape_costs: object " + std::to_string(objects[j]) + " is outside [0, objects)");
            return -1;
        }
        if (dims[2 * j] < 1 || dims[2 * j + 1] < 1 || dims[2 * j] > (1 << 20) || dims[2 * j + 1] > (1 << 20)) {
            set_error("rg_shape_costs: a table needs at least one angle and one distance (and at most 2^20 of either)");
            return -1;
        }
        if (!std::isfinite(centres[2 * j]) || !std::isfinite(centres[2 * j + 1]) || !std::isfinite(shifts[j])) {
            set_error("rg_shape_costs: centre and shift of an object must be finite");
            return -1;
        }
        offsets[j] = total;
        total += (long long)dims[2 * j] * dims[2 * j + 1];
    }
    hipStream_t st = rg->im->ctx->stream;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t n = (size_t)n_selected;
    const size_t o_obj = take(n * 4), o_cen = take(n * 16), o_shift = take(n * 8), o_dims = take(n * 8), o_offs = take(n * 8);
    const size_t o_tab = take((size_t)total * 8), o_proba = take(proba_out ? n * v.K * 8 : 0);
    if (rg->job.ensure(at)) return -1;
    unsigned char *dev = rg->job.as<unsigned char>();
    // every exit below waits for the stream: the copies read `offsets` and the caller's arrays until then
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(dev + o_obj, objects, n * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev + o_cen, centres, n * 16, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev + o_shift, shifts, n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev + o_dims, dims, n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev + o_offs, offsets.data(), n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev + o_tab, tables, (size_t)total * 8, hipMemcpyHostToDevice, st));
        RgShapeJob job;
        job.objects = reinterpret_cast<const int32_t *>(dev + o_obj);
        job.centres = reinterpret_cast<const double *>(dev + o_cen);
        job.shifts = reinterpret_cast<const double *>(dev + o_shift);
        job.dims = reinterpret_cast<const int32_t *>(dev + o_dims);
        job.offsets = reinterpret_cast<const long long *>(dev + o_offs);
        job.tables = reinterpret_cast<const double *>(dev + o_tab);
        job.proba = proba_out ? reinterpret_cast<double *>(dev + o_proba) : nullptr;
        if (launch_rg_shape_cost(v, job, n_selected, st)) return -1;
        if (proba_out) HIP_TRY(hipMemcpyAsync(proba_out, job.proba, n * v.K * 8, hipMemcpyDeviceToHost, st));
        return 0;
    };
    const int failed = run();
    if (failed) {
        (void)hipStreamSynchronize(st);
        return -1;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_rg_object_shapes(imsegm_rg *rg, const int32_t *labels, const int32_t *positions, const float *directions, int n_angles,
                            float *rays_out)
{
    if (rg_bind(rg)) return -1;
    if (!positions || !directions || !rays_out || n_angles < 1 || n_angles > 4096) {
        set_error("rg_object_shapes: positions, 1 to 4096 ray directions and a result array are required");
        return -1;
    }
    if (rg_put_labels(rg, labels)) return -1;
    const RgView &v = rg->v;
    hipStream_t st = rg->im->ctx->stream;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t o_pos = take((size_t)v.n_obj * 8), o_dir = take((size_t)n_angles * 8), o_out = take((size_t)v.n_obj * n_angles * 4);
    if (rg->job.ensure(at)) return -1;
    unsigned char *dev = rg->job.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + o_pos, positions, (size_t)v.n_obj * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_dir, directions, (size_t)n_angles * 8, hipMemcpyHostToDevice, st));
    if (launch_rg_object_rays(v, reinterpret_cast<const int32_t *>(dev + o_pos), reinterpret_cast<const float *>(dev + o_dir), n_angles,
                              reinterpret_cast<float *>(dev + o_out), st))
        return -1;
    HIP_TRY(hipMemcpyAsync(rays_out, dev + o_out, (size_t)v.n_obj * n_angles * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_rg_greedy_step(imsegm_rg *rg, const int32_t *labels, int allow_obj_swap, const double *coefs, int *n_out, int32_t *objects_out,
                          int32_t *superpixels_out, double *changes_out)
{
    if (rg_bind(rg)) return -1;
    RgCoefs c;
    if (rg_coefs(coefs, c)) return -1;
    if (!n_out || !objects_out || !superpixels_out) {
        set_error("rg_greedy_step: null result array");
        return -1;
    }
    if (rg_put_labels(rg, labels)) return -1;
    const RgView &v = rg->v;
    hipStream_t st = rg->im->ctx->stream;
    if (launch_rg_candidates(v, allow_obj_swap, st)) return -1;
    if (launch_rg_scores(v, c, changes_out != nullptr, st)) return -1;
    int32_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, v.slots + (size_t)v.n_obj * v.K, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (count < 0 || (size_t)count > (size_t)v.n_obj * v.K) {
        set_error("rg_greedy_step: candidate count out of range");
        return -1;
    }
    *n_out = count;
    if (count > 0) {
        HIP_TRY(hipMemcpyAsync(objects_out, v.cand_obj, (size_t)count * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(superpixels_out, v.cand_sp, (size_t)count * 4, hipMemcpyDeviceToHost, st));
        if (changes_out) HIP_TRY(hipMemcpyAsync(changes_out, v.cand_change, (size_t)count * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

int imsegm_rg_criterion(imsegm_rg *rg, const int32_t *labels, const double *coefs, double *criterion_out)
{
    if (rg_bind(rg)) return -1;
    RgCoefs c;
    if (rg_coefs(coefs, c)) return -1;
    if (!criterion_out) {
        set_error("rg_criterion: null result");
        return -1;
    }
    if (rg_put_labels(rg, labels)) return -1;
    hipStream_t st = rg->im->ctx->stream;
    if (launch_rg_crit(rg->v, c, st)) return -1;
    HIP_TRY(hipMemcpyAsync(criterion_out, rg->v.crit, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
