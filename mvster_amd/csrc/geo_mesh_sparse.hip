// Brick-sparse TSDF volumes on the GPU (the definition is tsdf_sparse_math.h): a scan meshed at the
// resolution of its depth maps.  Only the 8 x 8 x 8 bricks near a surface are stored; a dense int32 directory over the bricks of
// the virtual grid finds them.  Count -> scan -> emit everywhere, in the form of geo_mesh.hip; a tile is one brick.
//
//   mvster_tsdf_sparse_mark            sparse_mark_kernel       one lane per (view, pixel): 1 into the byte of every brick its slab
//                                                               touches (plain byte stores of equal values: the race is benign)
//   mvster_tsdf_sparse_compact_count   sparse_flags_kernel      counts [tile of 512 bricks], then mv_scan_counts: the last word of
//                                                               offsets is Nb, the ONE read-back of an allocation
//   mvster_tsdf_sparse_compact_emit    sparse_slots_kernel      brick_slot [nbricks] (-1 = absent) and bricks [Nb] ascending
//   mvster_tsdf_sparse_integrate       sparse_integrate_kernel  one workgroup of 512 lanes per allocated brick, a wave is an 8 x 8
//                                                               slice; the loop over ALL views runs inside the lane with the view
//                                                               rows read at wave-uniform addresses (tsdf::add_view)
//   mvster_mesh_sparse_count           sparse_nodes_kernel      edge_mask, rank [Nb, 512], vcounts [Nb]
//                                      sparse_cells_kernel      tcounts [Nb]; (mv_scan_counts) x 2: the last words of voffsets /
//                                                               toffsets are Nv and Nt, the ONE read-back of an extraction
//   mvster_mesh_sparse_emit_vertices   sparse_vertices_kernel   vertex (A, d) -> voffsets[brick] + rank[A] + popcount(mask below d)
//   mvster_mesh_sparse_emit_triangles  sparse_triangles_kernel  a cell ranks itself in its brick and finds every corner's vertex
//                                                               through the owner's brick: its offset, rank and mask
// Every extraction workgroup first stages the brick's 10 x 10 x 10 window of tsdf and weight in LDS (8 kB); tsdf::edge_mask,
// cell_valid and cell_inside run on it.  No atomics at all: two runs give the same bytes.
#include "common.hpp"
#include "tsdf_sparse_math.h"

namespace {

constexpr int kWG = tsdfs::kBrickNodes;       // 512 lanes: one per node of a brick
constexpr int kMarkWG = 256;

struct SparseArgs {
    tsdfs::Sparse s;
    const int* bricks;                // [Nb]
    const float* depth;               // [V, H, W]
    const unsigned char* mask;
    const unsigned char* images;      // [V, H, W, 3]
    const double* views;              // [V, 21]
    float* tsdf;                      // [Nb, 512]
    int* weight;
    unsigned char* rgb;               // [Nb, 512, 3]
    unsigned char* has_color;
    unsigned char* flags;             // [nbricks]
    int* slot_out;                    // [nbricks]
    int* bricks_out;                  // [Nb]
    unsigned char* edge_mask;         // [Nb, 512]
    unsigned short* rank;             // [Nb, 512]
    int* vcounts;                     // [Nb] (the compaction: [tiles])
    int* tcounts;
    const long* voffsets;             // [Nb + 1]
    const long* toffsets;
    float* vertices;                  // [Nv, 3]
    unsigned char* colors;
    long* keys;                       // [Nv] or null
    int* triangles;                   // [Nt, 3]
    double trunc;
    long pixels, Nv, Nt;
    int V, H, W, min_weight;
};

// the exclusive prefix of c over the workgroup's 512 lanes in lane order, and the workgroup's total (every lane calls this)
__device__ __forceinline__ int tile_prefix(int c, int* wave_total, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wave_total[wave] = x;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWG / 64; ++w) {
        if (w < wave) base += wave_total[w];
        total += wave_total[w];
    }
    return base + x - c;
}

__global__ void __launch_bounds__(kMarkWG) sparse_mark_kernel(SparseArgs a) {
    const long p = (long)blockIdx.x * kMarkWG + threadIdx.x;
    if (p >= a.pixels) return;
    if (a.mask[p] == 0) return;
    const long hw = (long)a.H * a.W;
    const int v = (int)(p / hw);
    const long r = p - (long)v * hw;
    const int py = (int)(r / a.W), px = (int)(r - (long)py * a.W);
    tsdfs::mark_pixel(a.s, a.views + (long)v * tsdf::kView, px, py, a.depth[p], a.trunc, a.flags);
}

__global__ void __launch_bounds__(kWG) sparse_flags_kernel(SparseArgs a) {
    __shared__ int wave_total[kWG / 64];
    const long b = (long)blockIdx.x * kWG + threadIdx.x;
    int total;
    tile_prefix(b < a.s.nbricks && a.flags[b] != 0 ? 1 : 0, wave_total, total);
    if (threadIdx.x == 0) a.vcounts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kWG) sparse_slots_kernel(SparseArgs a) {
    __shared__ int wave_total[kWG / 64];
    const long b = (long)blockIdx.x * kWG + threadIdx.x;
    const bool set = b < a.s.nbricks && a.flags[b] != 0;
    int total;
    const long at = a.voffsets[blockIdx.x] + tile_prefix(set ? 1 : 0, wave_total, total);
    if (b >= a.s.nbricks) return;
    const bool fits = set && at < a.s.Nb;                                       // capacity of the caller's buffer
    a.slot_out[b] = fits ? (int)at : -1;
    if (fits) a.bricks_out[at] = (int)b;
}

// the workgroup's brick, or false for a brick number outside the grid (a list that lies is not followed)
__device__ __forceinline__ bool brick_of(const SparseArgs& a, int& bi, int& bj, int& bk) {
    const long b = a.bricks[blockIdx.x];
    if ((unsigned long)b >= (unsigned long)a.s.nbricks) return false;
    tsdfs::brick_ijk(a.s, b, bi, bj, bk);
    return true;
}

__global__ void __launch_bounds__(kWG) sparse_integrate_kernel(SparseArgs a) {
    int bi = a.s.nbx, bj = a.s.nby, bk = a.s.nbz;                               // a bad brick number: every node is outside, weight 0
    brick_of(a, bi, bj, bk);
    tsdfs::integrate_node(a.s, bi, bj, bk, threadIdx.x, a.views, a.depth, a.mask, a.images, a.V, a.H, a.W, a.trunc,
                          (long)blockIdx.x * kWG + threadIdx.x, a.tsdf, a.weight, a.rgb, a.has_color);
}

// stages the window of the workgroup's brick -> false (for the whole workgroup) if the brick number is bad
__device__ __forceinline__ bool stage(const SparseArgs& a, float* wt, int* ww, int& bi, int& bj, int& bk) {
    const bool ok = brick_of(a, bi, bj, bk);
    if (ok) tsdfs::stage_window(a.s, bi, bj, bk, a.tsdf, a.weight, wt, ww, threadIdx.x, kWG);
    __syncthreads();
    return ok;
}

__global__ void __launch_bounds__(kWG) sparse_nodes_kernel(SparseArgs a) {
    __shared__ float wt[tsdfs::kWinNodes];
    __shared__ int ww[tsdfs::kWinNodes];
    __shared__ int wave_total[kWG / 64];
    int bi, bj, bk;
    const bool ok = stage(a, wt, ww, bi, bj, bk);
    const unsigned m = ok ? tsdfs::node_mask(wt, ww, a.min_weight, threadIdx.x) : 0u;
    int total;
    const int before = tile_prefix(tsdf::popcount8(m), wave_total, total);
    const long at = (long)blockIdx.x * kWG + threadIdx.x;
    a.edge_mask[at] = (unsigned char)m;
    a.rank[at] = (unsigned short)before;                                        // < 512 * 7
    if (threadIdx.x == 0) a.vcounts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kWG) sparse_cells_kernel(SparseArgs a) {
    __shared__ float wt[tsdfs::kWinNodes];
    __shared__ int ww[tsdfs::kWinNodes];
    __shared__ int wave_total[kWG / 64];
    int bi, bj, bk;
    const bool ok = stage(a, wt, ww, bi, bj, bk);
    unsigned in;
    int total;
    tile_prefix(ok ? tsdfs::cell_count(wt, ww, a.min_weight, threadIdx.x, in) : 0, wave_total, total);
    if (threadIdx.x == 0) a.tcounts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kWG) sparse_vertices_kernel(SparseArgs a) {
    __shared__ float wt[tsdfs::kWinNodes];
    __shared__ int ww[tsdfs::kWinNodes];
    int bi, bj, bk;
    if (!stage(a, wt, ww, bi, bj, bk)) return;
    const int l = threadIdx.x;
    const long at = (long)blockIdx.x * kWG + l;
    const unsigned m = a.edge_mask[at];
    if (!m) return;
    const long base = a.voffsets[blockIdx.x] + a.rank[at];
    const int wn = tsdfs::window_index(l);
    const tsdf::Grid w = tsdfs::window_grid();
    for (unsigned d = 1; d < 8u; ++d) {
        if (!((m >> d) & 1u)) continue;
        const long r = base + tsdf::edge_rank(m, d);
        if ((unsigned long)r >= (unsigned long)a.Nv) continue;                  // capacity of the caller's buffers
        float pos[3];
        unsigned char col[3];
        long key;
        tsdfs::vertex(a.s, bi, bj, bk, l, at, d, wt[wn], wt[wn + (int)tsdf::offset_index(w, d)], a.rgb, a.has_color, pos, col, key);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.vertices[r * 3 + c] = pos[c];
            a.colors[r * 3 + c] = col[c];
        }
        if (a.keys) a.keys[r] = key;
    }
}

__global__ void __launch_bounds__(kWG) sparse_triangles_kernel(SparseArgs a) {
    __shared__ float wt[tsdfs::kWinNodes];
    __shared__ int ww[tsdfs::kWinNodes];
    __shared__ int wave_total[kWG / 64];
    int bi, bj, bk;
    const bool ok = stage(a, wt, ww, bi, bj, bk);
    const int l = threadIdx.x;
    unsigned in = 0u;
    int total;
    const int count = ok ? tsdfs::cell_count(wt, ww, a.min_weight, l, in) : 0;
    long r = a.toffsets[blockIdx.x] + tile_prefix(count, wave_total, total);
    if (!count) return;
    for (int q = 0; q < 6; ++q) {
        const unsigned corners = tsdf::tet_corners(q);
        const unsigned cw = tsdf::tet_case(tsdf::tet_inside(in, corners));
        const bool mirrored = tsdf::tet_mirrored(q);
        const int tris = (int)(cw & 3u);
        for (int t = 0; t < tris; ++t, ++r) {
            if ((unsigned long)r >= (unsigned long)a.Nt) continue;              // capacity of the caller's buffer
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned lo, d;
                tsdf::edge_owner(corners, tsdf::triangle_edge(cw, mirrored, t, c), lo, d);
                const long owner = tsdfs::corner_at(a.s, bi, bj, bk, l, lo);    // a corner of a valid cell: stored
                a.triangles[r * 3 + c] =
                    owner < 0 ? -1 : (int)(a.voffsets[owner / kWG] + a.rank[owner] + tsdf::edge_rank(a.edge_mask[owner], d));
            }
        }
    }
}

bool finite_d(double x) { return x - x == 0.0; }

// the virtual grid, or false where it is refused
bool sparse_of(int nx, int ny, int nz, double ox, double oy, double oz, double voxel, const int* slot, long Nb, tsdfs::Sparse& s) {
    const long n = tsdfs::grid_bricks(nx, ny, nz);
    if (n < 0 || Nb < 0 || Nb > n) return false;
    if (!(voxel > 0.0) || !finite_d(voxel) || !finite_d(ox) || !finite_d(oy) || !finite_d(oz)) return false;
    s.g.nx = nx; s.g.ny = ny; s.g.nz = nz;
    s.g.ox = ox; s.g.oy = oy; s.g.oz = oz; s.g.voxel = voxel;
    s.nbx = (int)tsdfs::bricks_along(nx); s.nby = (int)tsdfs::bricks_along(ny); s.nbz = (int)tsdfs::bricks_along(nz);
    s.nbricks = n;
    s.Nb = Nb;
    s.slot = slot;
    return true;
}

bool maps_ok(int V, int H, int W, double trunc) {
    return V >= 1 && H >= 1 && W >= 1 && H <= tsdf::kMaxSide && W <= tsdf::kMaxSide && trunc > 0.0 && finite_d(trunc);
}

long flag_tiles(long nbricks) { return (nbricks + kWG - 1) / kWG; }

}  // namespace

extern "C" int mvster_tsdf_sparse_bricks(int nx, int ny, int nz) {
    const long n = tsdfs::grid_bricks(nx, ny, nz);                              // (at most 2^27: an int holds it)
    return n < 0 ? MVSTER_ERR_SHAPE : (int)n;
}

extern "C" int mvster_tsdf_sparse_mark(const float* depth, const unsigned char* mask, const double* views, int V, int H, int W,
                                       double ox, double oy, double oz, double voxel, int nx, int ny, int nz, double trunc,
                                       unsigned char* flags, void* stream) {
    if (!depth || !mask || !views || !flags) return MVSTER_ERR_NULL;
    SparseArgs a = {};
    if (!sparse_of(nx, ny, nz, ox, oy, oz, voxel, nullptr, 0, a.s) || !maps_ok(V, H, W, trunc)) return MVSTER_ERR_SHAPE;
    a.pixels = (long)V * H * W;                                                 // (< 2^71 cannot be: V < 2^31, H W <= 2^40 -> checked next)
    if ((long)H * W > (0x7fffffffl * (long)kMarkWG) / V) return MVSTER_ERR_SHAPE;
    a.depth = depth; a.mask = mask; a.views = views; a.flags = flags;
    a.trunc = trunc;
    a.V = V; a.H = H; a.W = W;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(flags, 0, (size_t)a.s.nbricks, st) != hipSuccess) return MVSTER_ERR_LAUNCH;
    hipLaunchKernelGGL(sparse_mark_kernel, dim3((unsigned)((a.pixels + kMarkWG - 1) / kMarkWG)), dim3(kMarkWG), 0, st, a);
    return mv_check_launch();
}

extern "C" int mvster_tsdf_sparse_compact_count(const unsigned char* flags, long nbricks, int* counts, long* offsets, void* stream) {
    if (!flags || !counts || !offsets) return MVSTER_ERR_NULL;
    if (nbricks < 1 || nbricks > tsdfs::kMaxBricks) return MVSTER_ERR_SHAPE;
    SparseArgs a = {};
    a.s.nbricks = nbricks;
    a.flags = const_cast<unsigned char*>(flags);
    a.vcounts = counts;
    const long tiles = flag_tiles(nbricks);
    hipLaunchKernelGGL(sparse_flags_kernel, dim3((unsigned)tiles), dim3(kWG), 0, (hipStream_t)stream, a);
    const int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    return mv_scan_counts(counts, offsets, tiles, (hipStream_t)stream);
}

extern "C" int mvster_tsdf_sparse_compact_emit(const unsigned char* flags, long nbricks, const long* offsets, long Nb, int* brick_slot,
                                               int* bricks, void* stream) {
    if (!flags || !offsets || !brick_slot) return MVSTER_ERR_NULL;
    if (nbricks < 1 || nbricks > tsdfs::kMaxBricks || Nb < 0 || Nb > nbricks) return MVSTER_ERR_SHAPE;
    if (Nb > 0 && !bricks) return MVSTER_ERR_NULL;
    SparseArgs a = {};
    a.s.nbricks = nbricks;
    a.s.Nb = Nb;
    a.flags = const_cast<unsigned char*>(flags);
    a.voffsets = offsets;
    a.slot_out = brick_slot;
    a.bricks_out = bricks;
    hipLaunchKernelGGL(sparse_slots_kernel, dim3((unsigned)flag_tiles(nbricks)), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}

extern "C" int mvster_tsdf_sparse_integrate(const float* depth, const unsigned char* mask, const unsigned char* images,
                                            const double* views, int V, int H, int W, double ox, double oy, double oz, double voxel,
                                            int nx, int ny, int nz, double trunc, const int* bricks, long Nb, float* tsdf_out,
                                            int* weight, unsigned char* rgb, unsigned char* has_color, void* stream) {
    if (!depth || !mask || !images || !views) return MVSTER_ERR_NULL;
    SparseArgs a = {};
    if (!sparse_of(nx, ny, nz, ox, oy, oz, voxel, nullptr, Nb, a.s) || !maps_ok(V, H, W, trunc)) return MVSTER_ERR_SHAPE;
    if (Nb == 0) return MVSTER_OK;                                              // no brick: nothing to write
    if (!bricks || !tsdf_out || !weight || !rgb || !has_color) return MVSTER_ERR_NULL;
    a.bricks = bricks; a.depth = depth; a.mask = mask; a.images = images; a.views = views;
    a.tsdf = tsdf_out; a.weight = weight; a.rgb = rgb; a.has_color = has_color;
    a.trunc = trunc;
    a.V = V; a.H = H; a.W = W;
    hipLaunchKernelGGL(sparse_integrate_kernel, dim3((unsigned)Nb), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}

extern "C" int mvster_mesh_sparse_count(const float* tsdf_in, const int* weight, const int* brick_slot, const int* bricks, long Nb,
                                        int nx, int ny, int nz, int min_weight, unsigned char* edge_mask, unsigned short* rank,
                                        int* vcounts, int* tcounts, long* voffsets, long* toffsets, void* stream) {
    if (!tsdf_in || !weight || !brick_slot || !bricks || !edge_mask || !rank || !vcounts || !tcounts || !voffsets || !toffsets)
        return MVSTER_ERR_NULL;
    SparseArgs a = {};
    if (!sparse_of(nx, ny, nz, 0.0, 0.0, 0.0, 1.0, brick_slot, Nb, a.s) || Nb < 1 || min_weight < 1) return MVSTER_ERR_SHAPE;
    a.bricks = bricks; a.tsdf = const_cast<float*>(tsdf_in); a.weight = const_cast<int*>(weight);
    a.edge_mask = edge_mask; a.rank = rank; a.vcounts = vcounts; a.tcounts = tcounts;
    a.min_weight = min_weight;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sparse_nodes_kernel, dim3((unsigned)Nb), dim3(kWG), 0, st, a);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(sparse_cells_kernel, dim3((unsigned)Nb), dim3(kWG), 0, st, a);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    rc = mv_scan_counts(vcounts, voffsets, Nb, st);
    if (rc != MVSTER_OK) return rc;
    return mv_scan_counts(tcounts, toffsets, Nb, st);
}

extern "C" int mvster_mesh_sparse_emit_vertices(const float* tsdf_in, const int* weight, const unsigned char* rgb,
                                                const unsigned char* has_color, const int* brick_slot, const int* bricks, long Nb,
                                                double ox, double oy, double oz, double voxel, int nx, int ny, int nz,
                                                const unsigned char* edge_mask, const unsigned short* rank, const long* voffsets,
                                                long Nv, float* vertices, unsigned char* colors, long* keys, void* stream) {
    if (!tsdf_in || !weight || !rgb || !has_color || !brick_slot || !bricks || !edge_mask || !rank || !voffsets) return MVSTER_ERR_NULL;
    SparseArgs a = {};
    if (!sparse_of(nx, ny, nz, ox, oy, oz, voxel, brick_slot, Nb, a.s) || Nb < 1 || Nv < 0 || Nv > 0x7fffffffl) return MVSTER_ERR_SHAPE;
    if (Nv == 0) return MVSTER_OK;                                              // no vertex: nothing to write
    if (!vertices || !colors) return MVSTER_ERR_NULL;
    a.bricks = bricks; a.tsdf = const_cast<float*>(tsdf_in); a.weight = const_cast<int*>(weight);
    a.rgb = const_cast<unsigned char*>(rgb); a.has_color = const_cast<unsigned char*>(has_color);
    a.edge_mask = const_cast<unsigned char*>(edge_mask); a.rank = const_cast<unsigned short*>(rank); a.voffsets = voffsets;
    a.vertices = vertices; a.colors = colors; a.keys = keys;
    a.Nv = Nv;
    hipLaunchKernelGGL(sparse_vertices_kernel, dim3((unsigned)Nb), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}

extern "C" int mvster_mesh_sparse_emit_triangles(const float* tsdf_in, const int* weight, const int* brick_slot, const int* bricks,
                                                 long Nb, int nx, int ny, int nz, int min_weight, const unsigned char* edge_mask,
                                                 const unsigned short* rank, const long* voffsets, const long* toffsets, long Nv,
                                                 long Nt, int* triangles, void* stream) {
    if (!tsdf_in || !weight || !brick_slot || !bricks || !edge_mask || !rank || !voffsets || !toffsets) return MVSTER_ERR_NULL;
    SparseArgs a = {};
    if (!sparse_of(nx, ny, nz, 0.0, 0.0, 0.0, 1.0, brick_slot, Nb, a.s) || Nb < 1 || min_weight < 1 || Nv < 0 || Nv > 0x7fffffffl ||
        Nt < 0)
        return MVSTER_ERR_SHAPE;
    if (Nt == 0) return MVSTER_OK;
    if (!triangles) return MVSTER_ERR_NULL;
    a.bricks = bricks; a.tsdf = const_cast<float*>(tsdf_in); a.weight = const_cast<int*>(weight);
    a.edge_mask = const_cast<unsigned char*>(edge_mask); a.rank = const_cast<unsigned short*>(rank);
    a.voffsets = voffsets; a.toffsets = toffsets; a.triangles = triangles;
    a.Nv = Nv; a.Nt = Nt;
    a.min_weight = min_weight;
    hipLaunchKernelGGL(sparse_triangles_kernel, dim3((unsigned)Nb), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}
