// Meshing a scan: volumetric fusion of depth maps into a truncated signed distance field on a dense
// grid, and the welded, indexed, coloured triangle mesh of its zero level by marching tetrahedra -- the definition, shared by
// geo_mesh.hip and the host build used only by the tests (tests/hostmath/tsdf_hostmath.cpp).  Like undistort_math.h: IEEE fp64,
// one correctly rounded operation per step in the order written, only + - * /, contraction switched off for both compilers,
// and no call into libm, so the kernels and the host build give the same bits.  It is this project's own definition,
// modelled on KinectFusion / Open3D-style integration; DESIGN.md lists the deviations.
//
// Grid: nx x ny x nz nodes (each >= 2, at most 2^31 - 1 in all), node (i, j, k) at origin + voxel (i, j, k) in fp64, linear
// index n = i + nx (j + ny k).
//
// Integration of a node p over the views v = 0 .. V-1 in view order.  A view is 21 doubles: K (9, row major; its third row is
// taken to be 0 0 1 and is not read), R (9, row major), t (3).
//   c_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a;  skip unless c_z > 0
//   u = ((K_00 c_x + K_01 c_y) + K_02 c_z) / c_z,  w = ((K_10 c_x + K_11 c_y) + K_12 c_z) / c_z
//   pixel (floor(u + 1/2), floor(w + 1/2));  skip unless 0 <= u + 1/2 < W and 0 <= w + 1/2 < H (a NaN skips)
//   d = depth[v, py, px] (float32);  skip if mask[v, py, px] == 0, d is not finite or d <= 0
//   sdf = d - c_z (the projective distance along z);  skip if sdf < -trunc
//   f = sdf / trunc, 1 where that exceeds 1;  sumF += f;  W += 1
//   if sdf <= trunc: the pixel's three bytes are added to three integer sums and C += 1
// -> tsdf = (float)(sumF / W) (1.0f for W = 0), weight = W, rgb_a = (2 sum_a + C) / (2 C) in integers (round half up; 0 for
// C = 0), has_color = (C > 0).  Every weight is 1: the one floating-point sum is sumF, added in view order.
//
// Surface.  A node is KNOWN if weight >= min_weight and INSIDE if tsdf < 0 (so tsdf == 0, and a NaN, count as outside).  The
// cell (i, j, k), i < nx-1, j < ny-1, k < nz-1, whose index is the index of its node (i, j, k), is VALID if its 8 corners are
// known.  Corner offsets are written as 3 bits, x = 1, y = 2, z = 4.  A cell is split into the six Freudenthal tetrahedra around
// the diagonal 0 -> 7, one per permutation (a, b, c) of the axes: corners (v0, v1, v2, v3) = (0, e_a, e_a + e_b, 7), in this
// order:
//     q   (a b c)   v1 v2   det[e_a e_b e_c]
//     0    x y z     1  3      +
//     1    x z y     1  5      -
//     2    y x z     2  3      -
//     3    y z x     2  6      +
//     4    z x y     4  5      +
//     5    z y x     4  6      -
// Along a tetrahedron the corner offsets grow as bit sets, so every edge of the triangulation runs from a node A to the node
// B = A + d, d in 1 .. 7 read as bits, and A OWNS it.  The cells that contain the edge (A, d) are A - s for the s in 0 .. 7 with
// s & d == 0: 4 for an axis edge, 2 for a face diagonal, 1 for the body diagonal; in each of them some tetrahedron has the
// edge, since every chain 0 < .. < 7 of bit sets is a tetrahedron.  The edge carries a vertex iff inside(A) != inside(B) and
// one of those cells is valid; edge_mask(A) has bit d set for it.
//   vertex (A, d): t = f_A / (f_A - f_B) in fp64 from the float32 values, position_a = (float)(p_A + t (p_B - p_A)) per axis,
//   colour_a = byte(c_A + t (c_B - c_A)) with byte(v) = (unsigned char)(v + 0.5) (round half up), where a node without a
//   colour takes the other end's (both without: 0).  It is computed from the owner in every cell that uses it, so all of them
//   see the same bytes: welding is by ownership, not by hashing.  With f_A == 0 (outside) and f_B < 0, t = 0 and the vertex is
//   the node itself; the triangles around it may have no area.  They are kept.
// Vertices are numbered by owner index, then d ascending.
//
// Triangles of a tetrahedron, from the inside mask m (bit p = v_p inside).  Its edges are numbered 0: v0v1, 1: v0v2, 2: v0v3,
// 3: v1v2, 4: v1v3, 5: v2v3.  For a tetrahedron with det > 0:
//     m        triangles (edge numbers)         m        triangles
//     0, 15    none
//     1        0 1 2                            14       0 2 1
//     2        0 4 3                            13       0 3 4
//     4        1 3 5                            11       1 5 3
//     8        2 5 4                             7       2 4 5
//     3        quad 1 2 4 3                     12       quad 1 3 4 2
//     5        quad 2 0 3 5                     10       quad 3 0 2 5
//     9        quad 0 1 5 4                      6       quad 0 4 5 1
// a quad (q0, q1, q2, q3) being the triangles (q0, q1, q2), (q0, q2, q3) -- the diagonal is q0 q2, fixed by the table.  For a
// tetrahedron with det < 0 the second and third corner of every triangle are exchanged.
// Why this is counter-clockwise seen from the outside (tsdf > 0) side: take det > 0 and v_i alone inside, and (i, j, k, l) an
// even permutation of (0, 1, 2, 3), so that (v_i, v_j, v_k, v_l) is positively oriented too.  The crossings on v_i v_j, v_i v_k,
// v_i v_l form a shrunken copy of the face (v_j, v_k, v_l), whose normal (v_k - v_j) x (v_l - v_j) points away from v_i for a
// positive tetrahedron: that is the first column with (i j k l) = (0 1 2 3), (1 0 3 2), (2 0 1 3), (3 0 2 1).  With v_i alone
// outside the normal must point toward v_i: the same triangle reversed (second column).  With v_i, v_j inside and (i, j, k, l)
// even, the crossings in the cyclic order ik, il, jl, jk bound a quadrilateral (neighbours share a face of the tetrahedron), and
// for v = (0, x, y, z), i j k l = 0 1 2 3 its normal is (0, +, +), toward the outside corners v_2, v_3: the rows 3, 5, 9 with
// (i j k l) = (0 1 2 3), (0 2 3 1), (0 3 1 2), and 12, 10, 6 with (2 3 0 1), (1 3 2 0), (1 2 0 3), each the reverse cycle of its
// complement.  A mirror image (det < 0) turns every triangle round.  The six tetrahedra of a cell and those of its neighbours
// meet face to face (the triangulation of a cell's face is the same from both sides: its diagonal runs from the lower corner),
// and on a shared face both sides compute the same two or three crossings, so the triangles join edge to edge with opposite
// directions: a surface that does not reach an invalid cell is a closed oriented 2-manifold.  The CPU test checks exactly that.
// Triangles are ordered by cell index, then q, then the order above.
#pragma once
#include "mvster_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace tsdf {

typedef unsigned long long u64;

constexpr int kView = 21;                 // doubles per view: K, R, t
constexpr long kMaxNodes = 0x7fffffffl;
constexpr long kMaxSide = 1l << 20;       // H, W at most

struct Grid {
    int nx, ny, nz;
    double ox, oy, oz, voxel;
};

MV_HD bool grid_ok(long nx, long ny, long nz) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > kMaxNodes || ny > kMaxNodes || nz > kMaxNodes) return false;
    if (nx * ny > kMaxNodes) return false;                                      // (< 2^62: no overflow)
    return nx * ny * nz <= kMaxNodes;
}

MV_HD long nodes_of(const Grid& g) { return (long)g.nx * g.ny * g.nz; }

MV_HD void node_ijk(const Grid& g, long n, int& i, int& j, int& k) {
    const unsigned u = (unsigned)n, row = u / (unsigned)g.nx;
    i = (int)(u - row * (unsigned)g.nx);
    k = (int)(row / (unsigned)g.ny);
    j = (int)(row - (unsigned)k * (unsigned)g.ny);
}

MV_HD long node_index(const Grid& g, int i, int j, int k) { return (long)i + (long)g.nx * ((long)j + (long)g.ny * (long)k); }

MV_HD double coord(double origin, double voxel, int i) { return origin + voxel * (double)i; }

MV_HD bool finite32(float x) { return x - x == 0.0f; }

// ---- integration ----------------------------------------------------------------------------------------------------------------------

struct Sums {
    double f;
    int w, c;
    unsigned r, g, b;
};

MV_HD Sums sums_empty() {
    Sums s;
    s.f = 0.0;
    s.w = s.c = 0;
    s.r = s.g = s.b = 0u;
    return s;
}

// one view m [kView] on the node (x, y, z); depth / mask [H,W], image [H,W,3] of that view
MV_HD void add_view(const double* m, const float* depth, const unsigned char* mask, const unsigned char* image, int H, int W,
                    double x, double y, double z, double trunc, Sums& s) {
    const double cx = ((m[9] * x + m[10] * y) + m[11] * z) + m[18];
    const double cy = ((m[12] * x + m[13] * y) + m[14] * z) + m[19];
    const double cz = ((m[15] * x + m[16] * y) + m[17] * z) + m[20];
    if (!(cz > 0.0)) return;
    const double u = (((m[0] * cx + m[1] * cy) + m[2] * cz) / cz) + 0.5;
    const double w = (((m[3] * cx + m[4] * cy) + m[5] * cz) / cz) + 0.5;
    if (!(u >= 0.0 && u < (double)W && w >= 0.0 && w < (double)H)) return;
    const long at = (long)w * W + (long)u;                                      // >= 0: truncation is the floor
    if (mask[at] == 0) return;
    const float d = depth[at];
    if (!finite32(d) || !(d > 0.0f)) return;
    const double sdf = (double)d - cz;
    if (sdf < -trunc) return;
    double f = sdf / trunc;
    if (f > 1.0) f = 1.0;
    s.f += f;
    s.w += 1;
    if (sdf <= trunc) {
        s.r += image[at * 3 + 0];
        s.g += image[at * 3 + 1];
        s.b += image[at * 3 + 2];
        s.c += 1;
    }
}

MV_HD float tsdf_of(const Sums& s) { return s.w > 0 ? (float)(s.f / (double)s.w) : 1.0f; }

MV_HD unsigned char mean_byte(unsigned sum, int c) { return c > 0 ? (unsigned char)((2u * sum + (unsigned)c) / (2u * (unsigned)c)) : (unsigned char)0; }

// ---- the surface ------------------------------------------------------------------------------------------------------------------------

MV_HD bool cell_valid(const Grid& g, const int* weight, int min_weight, int i, int j, int k) {
    if (i < 0 || j < 0 || k < 0 || i >= g.nx - 1 || j >= g.ny - 1 || k >= g.nz - 1) return false;
    const long n = node_index(g, i, j, k), sy = g.nx, sz = (long)g.nx * g.ny;
    return weight[n] >= min_weight && weight[n + 1] >= min_weight && weight[n + sy] >= min_weight &&
           weight[n + sy + 1] >= min_weight && weight[n + sz] >= min_weight && weight[n + sz + 1] >= min_weight &&
           weight[n + sz + sy] >= min_weight && weight[n + sz + sy + 1] >= min_weight;
}

MV_HD long offset_index(const Grid& g, unsigned d) {
    return (long)(d & 1u) + (long)g.nx * ((long)((d >> 1) & 1u) + (long)g.ny * (long)((d >> 2) & 1u));
}

// bit d (1 .. 7) set: the edge from node (i, j, k) to the node at offset d carries a vertex
MV_HD unsigned edge_mask(const Grid& g, const float* tsdf, const int* weight, int min_weight, int i, int j, int k) {
    unsigned valid = 0u;                                                        // bit s: the cell (i, j, k) - s is valid
    for (unsigned s = 0; s < 8u; ++s)
        if (cell_valid(g, weight, min_weight, i - (int)(s & 1u), j - (int)((s >> 1) & 1u), k - (int)((s >> 2) & 1u))) valid |= 1u << s;
    if (!valid) return 0u;
    const long n = node_index(g, i, j, k);
    const bool in = tsdf[n] < 0.0f;
    unsigned mask = 0u;
    for (unsigned d = 1; d < 8u; ++d) {
        unsigned any = 0u;
        for (unsigned s = 0; s < 8u; ++s)
            if ((s & d) == 0u) any |= (valid >> s) & 1u;
        if (any && (tsdf[n + offset_index(g, d)] < 0.0f) != in) mask |= 1u << d;      // (a valid cell holds B: it is in the grid)
    }
    return mask;
}

MV_HD int popcount8(unsigned m) {
    m = (m & 0x55u) + ((m >> 1) & 0x55u);
    m = (m & 0x33u) + ((m >> 2) & 0x33u);
    return (int)((m & 0x0fu) + (m >> 4));
}

// the rank of the vertex (A, d) among the vertices of its owner
MV_HD int edge_rank(unsigned mask, unsigned d) { return popcount8(mask & ((1u << d) - 1u)); }

MV_HD unsigned char to_byte(double v) {
    const double r = v + 0.5;
    return r >= 255.0 ? (unsigned char)255 : (r > 0.0 ? (unsigned char)r : (unsigned char)0);
}

// the vertex of the edge from node n = (i, j, k) to the node at offset d
MV_HD void vertex(const Grid& g, const float* tsdf, const unsigned char* rgb, const unsigned char* has_color, int i, int j, int k,
                   unsigned d, float* pos, unsigned char* col) {
    const long a = node_index(g, i, j, k), b = a + offset_index(g, d);
    const double fa = (double)tsdf[a], fb = (double)tsdf[b];
    const double t = fa / (fa - fb);
    const int di = (int)(d & 1u), dj = (int)((d >> 1) & 1u), dk = (int)((d >> 2) & 1u);
    const double ax = coord(g.ox, g.voxel, i), ay = coord(g.oy, g.voxel, j), az = coord(g.oz, g.voxel, k);
    pos[0] = (float)(ax + t * (coord(g.ox, g.voxel, i + di) - ax));
    pos[1] = (float)(ay + t * (coord(g.oy, g.voxel, j + dj) - ay));
    pos[2] = (float)(az + t * (coord(g.oz, g.voxel, k + dk) - az));
    const bool ha = has_color[a] != 0, hb = has_color[b] != 0;
    const long sa = ha ? a : b, sb = hb ? b : a;                                // a node without a colour takes the other end's
    for (int ch = 0; ch < 3; ++ch) {
        const double ca = (ha || hb) ? (double)rgb[sa * 3 + ch] : 0.0, cb = (ha || hb) ? (double)rgb[sb * 3 + ch] : 0.0;
        col[ch] = to_byte(ca + t * (cb - ca));
    }
}

// ---- the tables, packed into integers (no array is indexed at run time: nothing goes to scratch) ------------------------------------

// corner offsets of tetrahedron q, 3 bits each: v0 | v1 << 3 | v2 << 6 | v3 << 9
MV_HD unsigned tet_corners(int q) {
    const unsigned v1 = q < 2 ? 1u : (q < 4 ? 2u : 4u);
    const unsigned v2 = (0x656353u >> (4 * q)) & 7u;                            // 3 5 3 6 5 6, a nibble each
    return (v1 << 3) | (v2 << 6) | (7u << 9);
}

MV_HD bool tet_mirrored(int q) { return ((0x26u >> q) & 1u) != 0u; }              // q = 1, 2, 5: det < 0

// the ends (p, q) of edge e of a tetrahedron, 2 bits each
MV_HD unsigned edge_lo(unsigned e) { return (0x940u >> (2u * e)) & 3u; }          // 0 0 0 1 1 2
MV_HD unsigned edge_hi(unsigned e) { return (0xfb9u >> (2u * e)) & 3u; }          // 1 2 3 2 3 3

// the case word of an inside mask: triangles | q0 << 2 | q1 << 5 | q2 << 8 | q3 << 11
#define MV_TSDF_CASE(n, a, b, c, d) ((u64)((n) | ((a) << 2) | ((b) << 5) | ((c) << 8) | ((d) << 11)))
MV_HD unsigned tet_case(unsigned m) {
    const u64 w0 = MV_TSDF_CASE(0, 0, 0, 0, 0) | MV_TSDF_CASE(1, 0, 1, 2, 0) << 16 | MV_TSDF_CASE(1, 0, 4, 3, 0) << 32 |
                   MV_TSDF_CASE(2, 1, 2, 4, 3) << 48;                            // m = 0, 1, 2, 3
    const u64 w1 = MV_TSDF_CASE(1, 1, 3, 5, 0) | MV_TSDF_CASE(2, 2, 0, 3, 5) << 16 | MV_TSDF_CASE(2, 0, 4, 5, 1) << 32 |
                   MV_TSDF_CASE(1, 2, 4, 5, 0) << 48;                            // m = 4, 5, 6, 7
    const u64 w2 = MV_TSDF_CASE(1, 2, 5, 4, 0) | MV_TSDF_CASE(2, 0, 1, 5, 4) << 16 | MV_TSDF_CASE(2, 3, 0, 2, 5) << 32 |
                   MV_TSDF_CASE(1, 1, 5, 3, 0) << 48;                            // m = 8, 9, 10, 11
    const u64 w3 = MV_TSDF_CASE(2, 1, 3, 4, 2) | MV_TSDF_CASE(1, 0, 3, 4, 0) << 16 | MV_TSDF_CASE(1, 0, 2, 1, 0) << 32 |
                   MV_TSDF_CASE(0, 0, 0, 0, 0) << 48;                            // m = 12, 13, 14, 15
    const u64 w = m < 4u ? w0 : (m < 8u ? w1 : (m < 12u ? w2 : w3));
    return (unsigned)(w >> (16u * (m & 3u))) & 0xffffu;
}
#undef MV_TSDF_CASE

// bit c set: corner c of the cell at node n is inside
MV_HD unsigned cell_inside(const Grid& g, const float* tsdf, long n) {
    unsigned in = 0u;
    for (unsigned c = 0; c < 8u; ++c)
        if (tsdf[n + offset_index(g, c)] < 0.0f) in |= 1u << c;
    return in;
}

// the inside mask of tetrahedron q from the cell's
MV_HD unsigned tet_inside(unsigned in, unsigned corners) {
    return ((in >> (corners & 7u)) & 1u) | (((in >> ((corners >> 3) & 7u)) & 1u) << 1) | (((in >> ((corners >> 6) & 7u)) & 1u) << 2) |
           (((in >> ((corners >> 9) & 7u)) & 1u) << 3);
}

MV_HD int tet_triangles(unsigned in, int q) { return (int)(tet_case(tet_inside(in, tet_corners(q))) & 3u); }

// the triangles of a valid cell from its inside mask
MV_HD int cell_triangles(unsigned in) {
    if (in == 0u || in == 255u) return 0;
    int n = 0;
    for (int q = 0; q < 6; ++q) n += tet_triangles(in, q);
    return n;
}

// corner c = 0 .. 2 of triangle t (0 or 1) of a tetrahedron: the edge number in the tetrahedron
MV_HD unsigned triangle_edge(unsigned cw, bool mirrored, int t, int c) {
    int slot = c == 0 ? 0 : (c + t);                                            // (q0, q1, q2), (q0, q2, q3)
    if (mirrored && c != 0) slot = (c == 1 ? 2 : 1) + t;
    return (cw >> (2 + 3 * slot)) & 7u;
}

// edge e of the tetrahedron with `corners` in the cell at (i, j, k): its owner and its offset d
MV_HD void edge_owner(unsigned corners, unsigned e, unsigned& owner_offset, unsigned& d) {
    const unsigned lo = (corners >> (3u * edge_lo(e))) & 7u, hi = (corners >> (3u * edge_hi(e))) & 7u;
    owner_offset = lo;
    d = hi ^ lo;
}

}  // namespace tsdf
