// Host build of mvster_amd/csrc/tsdf_math.h -- TEST INFRASTRUCTURE ONLY.
// TSDF integration and marching tetrahedra with the very functions the kernels of geo_mesh.hip inline, as serial loops that
// follow the definition: nodes in index order, vertices by owner then d, triangles by cell, tetrahedron, triangle.  Never loaded
// by the product.  Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/mesh_cases.py).
#include "../../mvster_amd/csrc/tsdf_math.h"

namespace {

tsdf::Grid grid(int nx, int ny, int nz, double ox, double oy, double oz, double voxel) {
    tsdf::Grid g;
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.ox = ox; g.oy = oy; g.oz = oz; g.voxel = voxel;
    return g;
}

}  // namespace

extern "C" {

int hm_tsdf_grid_ok(long nx, long ny, long nz) { return tsdf::grid_ok(nx, ny, nz) ? 1 : 0; }

// depth / mask [V,H,W], images [V,H,W,3], views [V,21] -> tsdf, weight, rgb [n,3], has_color over the nodes
void hm_tsdf_integrate(const float* depth, const unsigned char* mask, const unsigned char* images, const double* views, int V, int H,
                       int W, double ox, double oy, double oz, double voxel, int nx, int ny, int nz, double trunc, float* out_tsdf,
                       int* weight, unsigned char* rgb, unsigned char* has_color) {
    const tsdf::Grid g = grid(nx, ny, nz, ox, oy, oz, voxel);
    const long nodes = tsdf::nodes_of(g), hw = (long)H * W;
    for (long n = 0; n < nodes; ++n) {
        int i, j, k;
        tsdf::node_ijk(g, n, i, j, k);
        const double x = tsdf::coord(ox, voxel, i), y = tsdf::coord(oy, voxel, j), z = tsdf::coord(oz, voxel, k);
        tsdf::Sums s = tsdf::sums_empty();
        for (int v = 0; v < V; ++v)
            tsdf::add_view(views + (long)v * tsdf::kView, depth + v * hw, mask + v * hw, images + v * hw * 3, H, W, x, y, z, trunc, s);
        out_tsdf[n] = tsdf::tsdf_of(s);
        weight[n] = s.w;
        rgb[n * 3 + 0] = tsdf::mean_byte(s.r, s.c);
        rgb[n * 3 + 1] = tsdf::mean_byte(s.g, s.c);
        rgb[n * 3 + 2] = tsdf::mean_byte(s.b, s.c);
        has_color[n] = s.c > 0 ? 1 : 0;
    }
}

// edge_mask [n] uint8, vbase [n] int64 (the number of the node's first vertex) -> counts[0] = vertices, counts[1] = triangles
void hm_tsdf_count(const float* f, const int* weight, int nx, int ny, int nz, int min_weight, unsigned char* edge_mask, long* vbase,
                   long* counts) {
    const tsdf::Grid g = grid(nx, ny, nz, 0.0, 0.0, 0.0, 1.0);
    const long nodes = tsdf::nodes_of(g);
    long nv = 0, nt = 0;
    for (long n = 0; n < nodes; ++n) {
        int i, j, k;
        tsdf::node_ijk(g, n, i, j, k);
        const unsigned m = tsdf::edge_mask(g, f, weight, min_weight, i, j, k);
        edge_mask[n] = (unsigned char)m;
        vbase[n] = nv;
        nv += tsdf::popcount8(m);
        if (tsdf::cell_valid(g, weight, min_weight, i, j, k)) nt += tsdf::cell_triangles(tsdf::cell_inside(g, f, n));
    }
    counts[0] = nv;
    counts[1] = nt;
}

// vertices [Nv,3], colors [Nv,3], owners [Nv,2] int64 = (owner node, d), triangles [Nt,3] with the buffers of hm_tsdf_count
void hm_tsdf_emit(const float* f, const int* weight, const unsigned char* rgb, const unsigned char* has_color, double ox, double oy,
                  double oz, double voxel, int nx, int ny, int nz, int min_weight, const unsigned char* edge_mask, const long* vbase,
                  float* vertices, unsigned char* colors, long* owners, int* triangles) {
    const tsdf::Grid g = grid(nx, ny, nz, ox, oy, oz, voxel);
    const long nodes = tsdf::nodes_of(g);
    long r = 0;
    for (long n = 0; n < nodes; ++n) {
        int i, j, k;
        tsdf::node_ijk(g, n, i, j, k);
        const unsigned m = edge_mask[n];
        for (unsigned d = 1; d < 8u; ++d) {
            if (!((m >> d) & 1u)) continue;
            const long at = vbase[n] + tsdf::edge_rank(m, d);
            tsdf::vertex(g, f, rgb, has_color, i, j, k, d, vertices + at * 3, colors + at * 3);
            owners[at * 2] = n;
            owners[at * 2 + 1] = (long)d;
        }
        if (!tsdf::cell_valid(g, weight, min_weight, i, j, k)) continue;
        const unsigned in = tsdf::cell_inside(g, f, n);
        for (int q = 0; q < 6; ++q) {
            const unsigned corners = tsdf::tet_corners(q);
            const unsigned cw = tsdf::tet_case(tsdf::tet_inside(in, corners));
            for (int t = 0; t < (int)(cw & 3u); ++t, ++r) {
                for (int c = 0; c < 3; ++c) {
                    unsigned lo, d;
                    tsdf::edge_owner(corners, tsdf::triangle_edge(cw, tsdf::tet_mirrored(q), t, c), lo, d);
                    const long owner = n + tsdf::offset_index(g, lo);
                    triangles[r * 3 + c] = (int)(vbase[owner] + tsdf::edge_rank(edge_mask[owner], d));
                }
            }
        }
    }
}

}  // extern "C"
