// api_forest.hip -- C ABI of the random-forest class model (include/imsegm_hip.h): the check of a packed forest on the host, its
// upload, and predict_proba on a host table (imsegm_forest_proba) or on the resident feature table of a session
// (imsegm_image2d_forest_proba); the kernels are in forest.hip
#include "forest.h"
#include "session.h"

namespace {

// Sizes, then every node: an inner node's children lie behind it and inside its tree (the left one is the next node), its feature
// is a column, a leaf's row is a row of leaf_values.  Children behind their parent make every walk strictly ascending, so it ends
// in the tree's last node at the latest, and that one has to be a leaf: no walk leaves the arrays, none comes back to a node.
int forest_check(const imsegm_forest *fo)
{
    if (!fo || !fo->nodes || !fo->tree_start || !fo->leaf_values) {
        set_error("forest: null argument");
        return -1;
    }
    auto refuse = [](const char *why) {
        set_error(std::string("forest: ") + why);
        return IMSEGM_E_FOREST_INPUT;
    };
    if (fo->n_classes < 1 || fo->n_classes > IMSEGM_FOREST_MAX_CLASSES) return refuse("1..16 classes");
    if (fo->n_features < 1 || fo->n_features > IMSEGM_FOREST_MAX_FEATURES) return refuse("1..256 features");
    if (fo->n_trees < 1 || fo->n_trees > IMSEGM_FOREST_MAX_TREES) return refuse("1..1024 trees");
    if (fo->n_nodes < fo->n_trees || fo->n_leaves < 1) return refuse("every tree has a node, and there is a leaf row");
    if (fo->tree_start[0] != 0 || fo->tree_start[fo->n_trees] != fo->n_nodes) return refuse("tree_start does not span the nodes");
    for (int t = 0; t < fo->n_trees; ++t) {
        const int first = fo->tree_start[t], last = fo->tree_start[t + 1];
        if (first < 0 || last > fo->n_nodes || last <= first || last - first > IMSEGM_FOREST_MAX_TREE_NODES)
            return refuse("a tree has between 1 and 2^23 nodes");
        const imsegm_forest_node *tree = fo->nodes + first;
        const int count = last - first;
        for (int i = 0; i < count; ++i) {
            const int32_t word = tree[i].word;
            if (word < 0) {
                if (~word >= fo->n_leaves) return refuse("a leaf row is out of range");
                continue;
            }
            const int right = word >> 8;
            if ((word & 0xff) >= fo->n_features) return refuse("a node's feature is out of range");
            if (i + 1 >= count || right <= i + 1 || right >= count)
                return refuse("a node index is out of range (children lie behind their parent, inside the tree)");
            if (!(tree[i].threshold == tree[i].threshold)) return refuse("a threshold is not a number");
        }
    }
    return 0;
}

// where the pieces of one call live inside the context's scratch (every piece starts on a 256-byte boundary).  The forest itself
// (nodes .. scaler) is one block: it is assembled at the same offsets in the page-locked staging block and goes up in one copy.
// table / proba / flag: the host-table call only -- a session reads its own table and keeps the result in a buffer of its own.
struct ForestPlan {
    size_t o_nodes = 0, o_start = 0, o_values = 0, o_scaler = 0, up_bytes = 0, o_z = 0, o_leaf = 0, o_table = 0, o_proba = 0, o_flag = 0, bytes = 0;
};
ForestPlan forest_plan(const imsegm_forest *fo, int n_rows, bool host_table)
{
    ForestPlan p;
    size_t at = 0;
    auto take = [&](size_t bytes) { size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    const size_t stride = forest_row_stride(n_rows);
    p.o_nodes = take((size_t)fo->n_nodes * sizeof(imsegm_forest_node));
    p.o_start = take((size_t)(fo->n_trees + 1) * 4);
    p.o_values = take((size_t)fo->n_leaves * fo->n_classes * 8);
    p.o_scaler = take((size_t)2 * fo->n_features * 8);
    p.up_bytes = at;
    p.o_z = take(stride * fo->n_features * 4);
    p.o_leaf = take(stride * fo->n_trees * 4);
    if (host_table) {
        p.o_table = take((size_t)n_rows * fo->n_features * 8);
        p.o_proba = take((size_t)n_rows * fo->n_classes * 8);
        p.o_flag = take(256);
    }
    p.bytes = at;
    return p;
}

// the forest into the context's scratch, and the launch chain on `table` (device) -> `proba`, `flag` (device; the flag is cleared here)
int forest_enqueue(imsegm_ctx *ctx, const imsegm_forest *fo, const ForestPlan &p, int n_rows, const double *table, double *proba,
                   int32_t *flag)
{
    hipStream_t st = ctx->stream;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    unsigned char *host = static_cast<unsigned char *>(ctx->stage(p.up_bytes));
    if (!host) {
        set_error("cannot allocate pinned staging memory");
        return -1;
    }
    const int F = fo->n_features;
    memcpy(host + p.o_nodes, fo->nodes, (size_t)fo->n_nodes * sizeof(imsegm_forest_node));
    memcpy(host + p.o_start, fo->tree_start, (size_t)(fo->n_trees + 1) * 4);
    memcpy(host + p.o_values, fo->leaf_values, (size_t)fo->n_leaves * fo->n_classes * 8);
    if (fo->scaler_mean) memcpy(host + p.o_scaler, fo->scaler_mean, (size_t)F * 8);
    if (fo->scaler_scale) memcpy(host + p.o_scaler + (size_t)F * 8, fo->scaler_scale, (size_t)F * 8);
    HIP_TRY(hipMemcpyAsync(dev, host, p.up_bytes, hipMemcpyHostToDevice, st));
    ctx->mark_stage_in_flight();
    HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
    ForestArgs a;
    a.n_rows = n_rows; a.F = F; a.C = fo->n_classes; a.T = fo->n_trees;
    a.stride = forest_row_stride(n_rows);
    a.table = table;
    a.mean = fo->scaler_mean ? reinterpret_cast<const double *>(dev + p.o_scaler) : nullptr;
    a.scale = fo->scaler_scale ? reinterpret_cast<const double *>(dev + p.o_scaler) + F : nullptr;
    a.leaf_values = reinterpret_cast<const double *>(dev + p.o_values);
    a.nodes = reinterpret_cast<const imsegm_forest_node *>(dev + p.o_nodes);
    a.tree_start = reinterpret_cast<const int32_t *>(dev + p.o_start);
    a.z = reinterpret_cast<float *>(dev + p.o_z);
    a.leaf = reinterpret_cast<int32_t *>(dev + p.o_leaf);
    a.proba = proba;
    a.flag = flag;
    const int sp = ctx->begin(PG_TERMS);
    if (launch_forest_proba(a, fo->n_leaves, st)) return -1;
    ctx->end(sp);
    return 0;
}

// wait, read the flag, and hand the probabilities out only when the table was taken
int forest_collect(imsegm_ctx *ctx, const int32_t *flag, const double *proba, size_t values, double *proba_out)
{
    hipStream_t st = ctx->stream;
    int32_t refused = 0;
    HIP_TRY(hipMemcpyAsync(&refused, flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (refused) {
        set_error(refused & 2 ? "forest: a walk did not end in a leaf" : "forest: the table holds a value that is not finite in float32");
        return IMSEGM_E_FOREST_INPUT;
    }
    HIP_TRY(hipMemcpyAsync(proba_out, proba, values * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" {

int imsegm_forest_proba(imsegm_ctx *ctx, const imsegm_forest *forest, const double *table, int n_rows, int n_columns, double *proba_out)
{
    if (bind(ctx)) return -1;
    if (int rc = forest_check(forest)) return rc;
    if (!table || !proba_out || n_rows < 0 || n_rows > (1 << 30)) {
        set_error("forest_proba: a table of 0 .. 2^30 rows and an output are required");
        return -1;
    }
    if (n_columns != forest->n_features) {
        set_error("forest_proba: the table does not have the columns the forest was fitted on");
        return -1;
    }
    if (n_rows == 0) return 0;
    const ForestPlan p = forest_plan(forest, n_rows, true);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    double *d_table = reinterpret_cast<double *>(dev + p.o_table), *d_proba = reinterpret_cast<double *>(dev + p.o_proba);
    int32_t *d_flag = reinterpret_cast<int32_t *>(dev + p.o_flag);
    HIP_TRY(hipMemcpyAsync(d_table, table, (size_t)n_rows * n_columns * 8, hipMemcpyHostToDevice, ctx->stream));
    if (forest_enqueue(ctx, forest, p, n_rows, d_table, d_proba, d_flag)) return -1;
    return forest_collect(ctx, d_flag, d_proba, (size_t)n_rows * forest->n_classes, proba_out);
}

int imsegm_image2d_forest_proba(imsegm_image2d *im, const imsegm_forest *forest, double *proba_out)
{
    if (!im || bind(im->ctx)) return -1;
    im->forest_ready = false;
    if (int rc = forest_check(forest)) return rc;
    if (!im->have_labels || im->feat_mask == 0 || im->feat_F < 1 || im->n_labels < 1) {
        set_error("forest_proba: no resident feature table (imsegm_image2d_features_color)");
        return -1;
    }
    if (im->feat_F != forest->n_features) {
        set_error("forest_proba: the resident table does not have the columns the forest was fitted on");
        return -1;
    }
    imsegm_ctx *ctx = im->ctx;
    const int K = im->n_labels, C = forest->n_classes;
    const ForestPlan p = forest_plan(forest, K, false);
    if (ctx->gc_buf.ensure(p.bytes) || im->forest.ensure(256 + (size_t)K * C * 8)) return -1;
    int32_t *d_flag = im->forest.as<int32_t>();
    double *d_proba = reinterpret_cast<double *>(im->forest.as<unsigned char>() + 256);
    if (forest_enqueue(ctx, forest, p, K, im->featK.as<double>(), d_proba, d_flag)) return -1;
    if (proba_out)
        if (int rc = forest_collect(ctx, d_flag, d_proba, (size_t)K * C, proba_out)) return rc;
    im->forest_ready = true;
    im->forest_K = K;
    im->forest_C = C;
    return 0;
}

}  // extern "C"
