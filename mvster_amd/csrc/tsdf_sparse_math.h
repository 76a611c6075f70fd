// Brick-sparse TSDF volumes: the definition, shared by geo_mesh_sparse.hip and the host build used only by
// the tests (tests/hostmath/tsdf_sparse_hostmath.cpp).  The rules of tsdf_math.h hold: IEEE fp64, one correctly rounded operation
// per step in the order written, only + - * /, contraction off, no libm.  Nothing of tsdf_math.h is changed; its functions are
// called on a brick's window where the bits allow, and the two value-taking forms below (vertex_values, node_at) restate the rest.
//
// Virtual grid.  origin, voxel and dims = (nx, ny, nz) as in tsdf_math.h, but each axis 2 .. 2^20 nodes and NO limit on their
// product: a global node number n = i + nx (j + ny k) is 64-bit (< 2^60).  A BRICK is 8 x 8 x 8 nodes: brick (bi, bj, bk) holds
// the nodes 8 b .. 8 b + 7 per axis, clipped to the grid; there are nbx = ceil(nx / 8) (.. nby, nbz) per axis, and its linear
// number is bi + nbx (bj + nby bk).  The DIRECTORY brick_slot [nbz, nby, nbx] int32 is dense over bricks, so the virtual grid may
// hold at most kMaxBricks = 2^27 of them (512 MB of directory; grid_ok checks it).  A sparse volume is an ascending list
// bricks [Nb] of allocated brick numbers (the set S), brick_slot[b] = its place in that list or -1, and brick-major storage
// tsdf / weight / has_color [Nb, 512], rgb [Nb, 512, 3]; a node's place in its brick is li + 8 (lj + 8 lk).
//
// Meaning.  A sparse volume with allocated set S IS the dense volume of tsdf_math.h on the same grid in which every node of a
// brick outside S has weight 0, tsdf 1.0f, rgb 0, has_color 0, and every node of a brick in S carries what tsdf::add_view over all
// views in view order gives it.  (Storage words of a partial brick beyond the grid hold the same empty values and are never
// read: node_at answers -1 for them.)  Its mesh is the dense extraction of that volume: the same validity (min_weight >= 1, so an
// absent node is unknown), edge ownership, vertex arithmetic (positions from coord(origin, voxel, GLOBAL i): the dense bits),
// case table and orientation.  This holds for ANY S.
//   Order: bricks ascending; vertices by (brick, local node number, d); triangles by (brick, local cell, q, the table's order).
//   Every vertex carries vertex_key = global owner node * 8 + d (int64), so a mesh can be compared with the dense one whatever
//   the order.
// How the extraction gets the dense bits: a workgroup (a host loop) stages the brick's WINDOW, the 10 x 10 x 10 nodes
// 8 b - 1 .. 8 b + 8 per axis, as tsdf and weight (8 kB), looking neighbouring bricks up through the directory; absent bricks
// and nodes outside the grid are staged as tsdf 1, weight 0.  The window is a 10 x 10 x 10 grid for tsdf::edge_mask, cell_valid and
// cell_inside: a node of the brick sits at window coordinates 1 .. 8, the cells around it at 0 .. 8, their corners at 0 .. 9, so
// every read stays inside, and a cell that leaves the real grid has a corner of weight 0 < min_weight: invalid, as in
// tsdf::cell_valid's range check.
//
// Which bricks are allocated (`allocate`; a definition, so that the GPU and the host give the same set).  For every view and
// every pixel (px, py) with mask != 0 and a finite depth d > 0 (float32, widened): the SLAB is the pixel's frustum, u in
// px -+ 1/2, w in py -+ 1/2, between camera z0 = max(d - trunc, 0) and z1 = d + trunc.  Its 8 corners (u, w, z) go back through the
// closed-form inverse of the upper-triangular K (K_10 is taken to be 0: the callers refuse another K) and through R^T (c - t):
//   c_y = ((w - K_12) z) / K_11;  c_x = (((u - K_02) z) - K_01 c_y) / K_00;  c_z = z;  e = c - t
//   X_a = ((R_0a e_x + R_1a e_y) + R_2a e_z);  node coordinate q_a = (X_a - origin_a) / voxel
// Their axis-aligned box [lo, hi] is widened by 2 nodes per side, and every brick the widened box touches, clipped to the grid,
// is allocated: per axis the bricks floor((lo - 2) / 8) .. floor((hi + 2) / 8) within 0 .. nb - 1 (none if the box misses the grid
// or a bound is not a number).
//
// COVERING PROPERTY.  Every node that some view counts with -trunc <= sdf <= trunc lies, together with its 26 neighbours, in
// allocated bricks.  Proof.  (1) Exact arithmetic, R orthonormal.  Let view v count node x with pixel (px, py), depth d and
// sdf = d - c_z in [-trunc, trunc], c = R x + t.  add_view demands c_z > 0, so c_z lies in [max(d - trunc, 0), d + trunc] =
// [z0, z1]; and floor(u + 1/2) = px, floor(w + 1/2) = py put the projection (u, w) into px -+ 1/2, py -+ 1/2.  So c lies in the set
// { z A (u, w, 1) : (u, w) in the pixel's square, z in [z0, z1] } with A = K^-1: a cone over a parallelogram cut by two planes
// of constant z, which is convex and is the hull of its 8 corners.  x = R^T (c - t) and q = (x - origin) / voxel are affine,
// so q lies in the box of the 8 transformed corners, [lo, hi].  x is a node, so q is a vector of integers; its 26 neighbours
// are q + {-1, 0, 1}^3, inside [lo - 1, hi + 1]: that is the first node of the widening.  (2) Rounding.  The second node must
// cover every difference between the numbers above and the computed ones, in node units.  (a) add_view rounds c, u, w, sdf: it
// may count a node whose exact c misses the slab by a few ulps of the quantities involved.  Each of its results is a sum of
// at most 4 products followed by one division and one addition, so its relative error is below 8 * 2^-53 of the magnitudes
// |R x| + |t| (for c) and |K c| / c_z (for u, w); moved back to the node, that is a displacement below 2^-48 (|x| + |t| + z1 / f
// * (W + H)) / voxel nodes (f = the smaller of |K_00|, |K_11|).  (b) The corners are computed with at most 12 rounded operations
// each: below 16 * 2^-53 (|c| + |t| + |origin|) / voxel nodes.  (c) R is orthonormal only as far as its fp64 (or widened fp32)
// entries allow: with E = max |R^T R - I|, x' = R^T (R x + t - t) = x + (R^T R - I) x is off by at most 3 E |x| / voxel nodes.
// So the property holds whenever  (2^-47 (|x| + |t| + |origin| + z1 (W + H) / f) + 3 E |x|) / voxel <= 1  for every node x of the
// grid: with all lengths below 2^40 voxels and E below 2^-22 (2^-20 / the grid's greatest coordinate in voxels) it is far inside.
// mesh.allocate_bricks checks the E term per view (3 E max|x| <= voxel / 4) and refuses a K with K_10 != 0 or K_00 K_11 == 0; the
// first term needs coordinates above 2^44 voxels to matter.  The floors that turn [lo - 2, hi + 2] into brick ranges are exact
// (a truncating conversion of a non-negative double below 2^21).  QED.
// CONSEQUENCE.  With S = allocate(...) and any min_weight >= 1 the sparse mesh is the dense mesh of the same grid, key for key
// and byte for byte.  A cell with a sign change has an inside corner A: tsdf_A < 0 means weight_A >= 1 and a mean of f below 0,
// so some view counted A with f < 0, i.e. -trunc <= sdf < 0.  All 8 corners of the cell are among A and its 26 neighbours, so
// they lie in allocated bricks and carry their dense values: the cell is the dense cell.  A vertex's owner and other end are
// corners of such a cell, and an edge carries a vertex iff its ends differ in sign and a cell around it is valid: such a cell
// has an inside corner, so it is valid in both volumes or in neither.  The other way round, a cell that is valid in the sparse
// volume has 8 corners of weight >= min_weight >= 1, all in S, all with their dense values.  Cells without an inside corner
// produce nothing in either volume.
#pragma once
#include "tsdf_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace tsdfs {

constexpr int kBrick = 8;
constexpr int kBrickNodes = 512;
constexpr int kWin = 10;
constexpr int kWinNodes = 1000;
constexpr long kMaxAxis = 1l << 20;          // nodes per axis of the virtual grid
constexpr long kMaxBricks = 1l << 27;        // bricks of the virtual grid: the directory is dense over them

// the virtual grid with its directory; slot may be null where only the geometry is used
struct Sparse {
    tsdf::Grid g;
    int nbx, nby, nbz;
    long nbricks;                             // nbx nby nbz
    long Nb;                                  // allocated bricks
    const int* slot;                          // [nbricks]: place in bricks, or -1
};

MV_HD long bricks_along(long n) { return (n + kBrick - 1) / kBrick; }

// the number of bricks of the virtual grid, or -1 where it is refused
MV_HD long grid_bricks(long nx, long ny, long nz) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > kMaxAxis || ny > kMaxAxis || nz > kMaxAxis) return -1;
    const long n = bricks_along(nx) * bricks_along(ny) * bricks_along(nz);      // (< 2^51: no overflow)
    return n <= kMaxBricks ? n : -1;
}

MV_HD void brick_ijk(const Sparse& s, long b, int& bi, int& bj, int& bk) {
    const unsigned u = (unsigned)b, row = u / (unsigned)s.nbx;
    bi = (int)(u - row * (unsigned)s.nbx);
    bk = (int)(row / (unsigned)s.nby);
    bj = (int)(row - (unsigned)bk * (unsigned)s.nby);
}

MV_HD long global_node(const Sparse& s, int i, int j, int k) { return (long)i + (long)s.g.nx * ((long)j + (long)s.g.ny * (long)k); }

// where the node (i, j, k) of the virtual grid is stored: slot * 512 + its place in the brick, or -1 for a node outside the grid
// or in an absent brick
MV_HD long node_at(const Sparse& s, int i, int j, int k) {
    if (i < 0 || j < 0 || k < 0 || i >= s.g.nx || j >= s.g.ny || k >= s.g.nz) return -1;
    const long b = (long)(i >> 3) + (long)s.nbx * ((long)(j >> 3) + (long)s.nby * (long)(k >> 3));
    const long at = s.slot[b];
    if ((unsigned long)at >= (unsigned long)s.Nb) return -1;                    // -1 = absent (and a directory that lies is not followed)
    return at * kBrickNodes + (long)((i & 7) + 8 * ((j & 7) + 8 * (k & 7)));
}

// ---- allocation ------------------------------------------------------------------------------------------------------------------------

// one slab corner (u, w, z) of view m in node coordinates
MV_HD void corner_nodes(const double* m, const tsdf::Grid& g, double u, double w, double z, double* q) {
    const double cy = ((w - m[5]) * z) / m[4];
    const double cx = (((u - m[2]) * z) - m[1] * cy) / m[0];
    const double ex = cx - m[18], ey = cy - m[19], ez = z - m[20];
    q[0] = ((((m[9] * ex + m[12] * ey) + m[15] * ez)) - g.ox) / g.voxel;
    q[1] = ((((m[10] * ex + m[13] * ey) + m[16] * ez)) - g.oy) / g.voxel;
    q[2] = ((((m[11] * ex + m[14] * ey) + m[17] * ez)) - g.oz) / g.voxel;
}

// the bricks lo .. hi (node coordinates, not yet widened) touch along an axis of n nodes -> false if none
MV_HD bool brick_range(double lo, double hi, int n, int& b0, int& b1) {
    lo = lo - 2.0;
    hi = hi + 2.0;
    if (!(lo <= hi) || !(hi >= 0.0) || !(lo <= (double)(n - 1))) return false;    // (a NaN fails the first test)
    if (hi > (double)(n - 1)) hi = (double)(n - 1);
    b0 = lo > 0.0 ? (int)((long)lo >> 3) : 0;                                   // truncation of a value in 0 .. 2^20 is the floor
    b1 = (int)((long)hi >> 3);
    return true;
}

// the brick ranges of pixel (px, py) of view m with depth d (mask already looked at) -> false if it allocates nothing
MV_HD bool pixel_bricks(const double* m, const tsdf::Grid& g, int px, int py, float d, double trunc, int* b0, int* b1) {
    if (!tsdf::finite32(d) || !(d > 0.0f)) return false;
    const double z1 = (double)d + trunc;
    double z0 = (double)d - trunc;
    if (!(z0 > 0.0)) z0 = 0.0;
    double lo[3], hi[3];
    bool bad = false;
    for (int c = 0; c < 8; ++c) {
        double q[3];
        corner_nodes(m, g, (double)px + ((c & 1) ? 0.5 : -0.5), (double)py + ((c & 2) ? 0.5 : -0.5), (c & 4) ? z1 : z0, q);
        for (int a = 0; a < 3; ++a) {
            if (!(q[a] - q[a] == 0.0)) bad = true;                              // an overflow: the pixel allocates nothing
            if (c == 0 || q[a] < lo[a]) lo[a] = q[a];
            if (c == 0 || q[a] > hi[a]) hi[a] = q[a];
        }
    }
    return !bad && brick_range(lo[0], hi[0], g.nx, b0[0], b1[0]) && brick_range(lo[1], hi[1], g.ny, b0[1], b1[1]) &&
           brick_range(lo[2], hi[2], g.nz, b0[2], b1[2]);
}

// flags [nbricks] uint8: 1 for every brick the pixel allocates (equal values from every writer)
MV_HD void mark_pixel(const Sparse& s, const double* m, int px, int py, float d, double trunc, unsigned char* flags) {
    int b0[3], b1[3];
    if (!pixel_bricks(m, s.g, px, py, d, trunc, b0, b1)) return;
    for (int bk = b0[2]; bk <= b1[2]; ++bk)                                     // (each range lies in 0 .. nb - 1)
        for (int bj = b0[1]; bj <= b1[1]; ++bj)
            for (int bi = b0[0]; bi <= b1[0]; ++bi) flags[(long)bi + (long)s.nbx * ((long)bj + (long)s.nby * (long)bk)] = 1;
}

// ---- integration -----------------------------------------------------------------------------------------------------------------------

// node l = li + 8 (lj + 8 lk) of brick (bi, bj, bk) over all views, written to place `at` of the brick-major arrays
MV_HD void integrate_node(const Sparse& s, int bi, int bj, int bk, int l, const double* views, const float* depth,
                          const unsigned char* mask, const unsigned char* images, int V, int H, int W, double trunc, long at,
                          float* out_tsdf, int* weight, unsigned char* rgb, unsigned char* has_color) {
    const int i = 8 * bi + (l & 7), j = 8 * bj + ((l >> 3) & 7), k = 8 * bk + (l >> 6);
    tsdf::Sums sm = tsdf::sums_empty();
    if (i < s.g.nx && j < s.g.ny && k < s.g.nz) {
        const double x = tsdf::coord(s.g.ox, s.g.voxel, i), y = tsdf::coord(s.g.oy, s.g.voxel, j), z = tsdf::coord(s.g.oz, s.g.voxel, k);
        const long hw = (long)H * W;
        for (int v = 0; v < V; ++v)
            tsdf::add_view(views + (long)v * tsdf::kView, depth + v * hw, mask + v * hw, images + v * hw * 3, H, W, x, y, z, trunc, sm);
    }
    out_tsdf[at] = tsdf::tsdf_of(sm);
    weight[at] = sm.w;
    rgb[at * 3 + 0] = tsdf::mean_byte(sm.r, sm.c);
    rgb[at * 3 + 1] = tsdf::mean_byte(sm.g, sm.c);
    rgb[at * 3 + 2] = tsdf::mean_byte(sm.b, sm.c);
    has_color[at] = sm.c > 0 ? 1 : 0;
}

// ---- the window --------------------------------------------------------------------------------------------------------------------------

MV_HD tsdf::Grid window_grid() {
    tsdf::Grid w;
    w.nx = w.ny = w.nz = kWin;
    w.ox = w.oy = w.oz = 0.0;
    w.voxel = 1.0;
    return w;
}

// entries first, first + step, .. of the window of brick (bi, bj, bk): wt / ww [1000]
MV_HD void stage_window(const Sparse& s, int bi, int bj, int bk, const float* f, const int* weight, float* wt, int* ww, int first,
                        int step) {
    for (int e = first; e < kWinNodes; e += step) {
        const int wk = e / 100, r = e - wk * 100, wj = r / 10, wi = r - wj * 10;
        const long at = node_at(s, 8 * bi + wi - 1, 8 * bj + wj - 1, 8 * bk + wk - 1);
        wt[e] = at >= 0 ? f[at] : 1.0f;
        ww[e] = at >= 0 ? weight[at] : 0;
    }
}

MV_HD int window_index(int l) { return ((l & 7) + 1) + kWin * ((((l >> 3) & 7) + 1) + kWin * ((l >> 6) + 1)); }

// tsdf::edge_mask of the brick's node l on the staged window
MV_HD unsigned node_mask(const float* wt, const int* ww, int min_weight, int l) {
    return tsdf::edge_mask(window_grid(), wt, ww, min_weight, (l & 7) + 1, ((l >> 3) & 7) + 1, (l >> 6) + 1);
}

// the triangles of the cell at the brick's node l, and its inside mask
MV_HD int cell_count(const float* wt, const int* ww, int min_weight, int l, unsigned& in) {
    in = 0u;
    const tsdf::Grid w = window_grid();
    if (!tsdf::cell_valid(w, ww, min_weight, (l & 7) + 1, ((l >> 3) & 7) + 1, (l >> 6) + 1)) return 0;
    in = tsdf::cell_inside(w, wt, window_index(l));
    return tsdf::cell_triangles(in);
}

// tsdf::vertex from values: the ends' tsdf (widened), coordinates, colour flags and colours
MV_HD void vertex_values(double fa, double fb, double ax, double bx, double ay, double by, double az, double bz, bool ha, bool hb,
                         const unsigned char* ca, const unsigned char* cb, float* pos, unsigned char* col) {
    const double t = fa / (fa - fb);
    pos[0] = (float)(ax + t * (bx - ax));
    pos[1] = (float)(ay + t * (by - ay));
    pos[2] = (float)(az + t * (bz - az));
    const unsigned char* sa = ha ? ca : cb;                                     // a node without a colour takes the other end's
    const unsigned char* sb = hb ? cb : ca;
    for (int ch = 0; ch < 3; ++ch) {
        const double va = (ha || hb) ? (double)sa[ch] : 0.0, vb = (ha || hb) ? (double)sb[ch] : 0.0;
        col[ch] = tsdf::to_byte(va + t * (vb - va));
    }
}

// the vertex (A, d), A = node l of brick (bi, bj, bk) stored at `at`; fb = the other end's tsdf from the window
MV_HD void vertex(const Sparse& s, int bi, int bj, int bk, int l, long at, unsigned d, float fa, float fb, const unsigned char* rgb,
                  const unsigned char* has_color, float* pos, unsigned char* col, long& key) {
    const int i = 8 * bi + (l & 7), j = 8 * bj + ((l >> 3) & 7), k = 8 * bk + (l >> 6);
    const int di = (int)(d & 1u), dj = (int)((d >> 1) & 1u), dk = (int)((d >> 2) & 1u);
    long bt = node_at(s, i + di, j + dj, k + dk);
    if (bt < 0) bt = at;                                                        // (cannot happen: B is a corner of a valid cell)
    vertex_values((double)fa, (double)fb, tsdf::coord(s.g.ox, s.g.voxel, i), tsdf::coord(s.g.ox, s.g.voxel, i + di),
                  tsdf::coord(s.g.oy, s.g.voxel, j), tsdf::coord(s.g.oy, s.g.voxel, j + dj), tsdf::coord(s.g.oz, s.g.voxel, k),
                  tsdf::coord(s.g.oz, s.g.voxel, k + dk), has_color[at] != 0, has_color[bt] != 0, rgb + at * 3, rgb + bt * 3, pos, col);
    key = global_node(s, i, j, k) * 8 + (long)d;
}

// the storage place of corner `lo` (3 bits) of the cell at node l of brick (bi, bj, bk), or -1 (cannot happen for a valid cell)
MV_HD long corner_at(const Sparse& s, int bi, int bj, int bk, int l, unsigned lo) {
    return node_at(s, 8 * bi + (l & 7) + (int)(lo & 1u), 8 * bj + ((l >> 3) & 7) + (int)((lo >> 1) & 1u), 8 * bk + (l >> 6) + (int)((lo >> 2) & 1u));
}

}  // namespace tsdfs
