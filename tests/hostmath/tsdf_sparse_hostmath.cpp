// Host build of mvster_amd/csrc/tsdf_sparse_math.h -- TEST INFRASTRUCTURE ONLY.
// Brick allocation, brick-major TSDF integration and the brick-tiled marching tetrahedra with the very functions the kernels of
// geo_mesh_sparse.hip inline, as serial loops that follow the definition: bricks ascending, vertices by (brick, local node, d),
// triangles by (brick, local cell, q, the table's order).  Never loaded by the product.
// Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/mesh_sparse_cases.py).
#include "../../mvster_amd/csrc/tsdf_sparse_math.h"

namespace {

tsdfs::Sparse sparse(int nx, int ny, int nz, double ox, double oy, double oz, double voxel, const int* slot, long Nb) {
    tsdfs::Sparse s;
    s.g.nx = nx; s.g.ny = ny; s.g.nz = nz;
    s.g.ox = ox; s.g.oy = oy; s.g.oz = oz; s.g.voxel = voxel;
    s.nbx = (int)tsdfs::bricks_along(nx); s.nby = (int)tsdfs::bricks_along(ny); s.nbz = (int)tsdfs::bricks_along(nz);
    s.nbricks = (long)s.nbx * s.nby * s.nbz;
    s.Nb = Nb;
    s.slot = slot;
    return s;
}

}  // namespace

extern "C" {

long hm_sparse_grid_bricks(long nx, long ny, long nz) { return tsdfs::grid_bricks(nx, ny, nz); }

// flags [nbricks] uint8 (zeroed by the caller) <- 1 for every allocated brick
void hm_sparse_mark(const float* depth, const unsigned char* mask, const double* views, int V, int H, int W, double ox, double oy,
                    double oz, double voxel, int nx, int ny, int nz, double trunc, unsigned char* flags) {
    const tsdfs::Sparse s = sparse(nx, ny, nz, ox, oy, oz, voxel, nullptr, 0);
    for (int v = 0; v < V; ++v)
        for (int py = 0; py < H; ++py)
            for (int px = 0; px < W; ++px) {
                const long at = ((long)v * H + py) * W + px;
                if (mask[at] != 0) tsdfs::mark_pixel(s, views + (long)v * tsdf::kView, px, py, depth[at], trunc, flags);
            }
}

// the brick-major volume of the bricks [Nb]
void hm_sparse_integrate(const float* depth, const unsigned char* mask, const unsigned char* images, const double* views, int V, int H,
                         int W, double ox, double oy, double oz, double voxel, int nx, int ny, int nz, double trunc, const int* bricks,
                         long Nb, float* out_tsdf, int* weight, unsigned char* rgb, unsigned char* has_color) {
    const tsdfs::Sparse s = sparse(nx, ny, nz, ox, oy, oz, voxel, nullptr, Nb);
    for (long r = 0; r < Nb; ++r) {
        int bi, bj, bk;
        tsdfs::brick_ijk(s, bricks[r], bi, bj, bk);
        for (int l = 0; l < tsdfs::kBrickNodes; ++l)
            tsdfs::integrate_node(s, bi, bj, bk, l, views, depth, mask, images, V, H, W, trunc, r * tsdfs::kBrickNodes + l, out_tsdf, weight,
                                  rgb, has_color);
    }
}

// edge_mask [Nb * 512] uint8, vbase [Nb * 512] int64 (the number of the node's first vertex) -> counts[0] = vertices, [1] = triangles
void hm_sparse_count(const float* f, const int* weight, const int* slot, const int* bricks, long Nb, int nx, int ny, int nz,
                     int min_weight, unsigned char* edge_mask, long* vbase, long* counts) {
    const tsdfs::Sparse s = sparse(nx, ny, nz, 0.0, 0.0, 0.0, 1.0, slot, Nb);
    float wt[tsdfs::kWinNodes];
    int ww[tsdfs::kWinNodes];
    long nv = 0, nt = 0;
    for (long r = 0; r < Nb; ++r) {
        int bi, bj, bk;
        tsdfs::brick_ijk(s, bricks[r], bi, bj, bk);
        tsdfs::stage_window(s, bi, bj, bk, f, weight, wt, ww, 0, 1);
        for (int l = 0; l < tsdfs::kBrickNodes; ++l) {
            const unsigned m = tsdfs::node_mask(wt, ww, min_weight, l);
            edge_mask[r * tsdfs::kBrickNodes + l] = (unsigned char)m;
            vbase[r * tsdfs::kBrickNodes + l] = nv;
            nv += tsdf::popcount8(m);
            unsigned in;
            nt += tsdfs::cell_count(wt, ww, min_weight, l, in);
        }
    }
    counts[0] = nv;
    counts[1] = nt;
}

// vertices [Nv,3], colors [Nv,3], keys [Nv] int64, triangles [Nt,3] with the buffers of hm_sparse_count
void hm_sparse_emit(const float* f, const int* weight, const unsigned char* rgb, const unsigned char* has_color, const int* slot,
                    const int* bricks, long Nb, double ox, double oy, double oz, double voxel, int nx, int ny, int nz, int min_weight,
                    const unsigned char* edge_mask, const long* vbase, float* vertices, unsigned char* colors, long* keys,
                    int* triangles) {
    const tsdfs::Sparse s = sparse(nx, ny, nz, ox, oy, oz, voxel, slot, Nb);
    float wt[tsdfs::kWinNodes];
    int ww[tsdfs::kWinNodes];
    long t_at = 0;
    for (long r = 0; r < Nb; ++r) {
        int bi, bj, bk;
        tsdfs::brick_ijk(s, bricks[r], bi, bj, bk);
        tsdfs::stage_window(s, bi, bj, bk, f, weight, wt, ww, 0, 1);
        for (int l = 0; l < tsdfs::kBrickNodes; ++l) {
            const long at = r * tsdfs::kBrickNodes + l;
            const unsigned m = edge_mask[at];
            const int wn = tsdfs::window_index(l);
            for (unsigned d = 1; d < 8u; ++d) {
                if (!((m >> d) & 1u)) continue;
                const long v = vbase[at] + tsdf::edge_rank(m, d);
                tsdfs::vertex(s, bi, bj, bk, l, at, d, wt[wn], wt[wn + tsdf::offset_index(tsdfs::window_grid(), d)], rgb, has_color,
                              vertices + v * 3, colors + v * 3, keys[v]);
            }
            unsigned in;
            if (!tsdfs::cell_count(wt, ww, min_weight, l, in)) continue;
            for (int q = 0; q < 6; ++q) {
                const unsigned corners = tsdf::tet_corners(q);
                const unsigned cw = tsdf::tet_case(tsdf::tet_inside(in, corners));
                for (int t = 0; t < (int)(cw & 3u); ++t, ++t_at) {
                    for (int c = 0; c < 3; ++c) {
                        unsigned lo, d;
                        tsdf::edge_owner(corners, tsdf::triangle_edge(cw, tsdf::tet_mirrored(q), t, c), lo, d);
                        const long owner = tsdfs::corner_at(s, bi, bj, bk, l, lo);
                        triangles[t_at * 3 + c] = owner < 0 ? -1 : (int)(vbase[owner] + tsdf::edge_rank(edge_mask[owner], d));
                    }
                }
            }
        }
    }
}

}  // extern "C"
