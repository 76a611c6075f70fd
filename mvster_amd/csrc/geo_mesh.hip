// Meshing a scan on the GPU (the definition is tsdf_math.h): all depth maps of a scan fused into a
// truncated signed distance field on a dense grid, and the welded, indexed, coloured mesh of its zero level by marching
// tetrahedra, in the count -> scan -> emit form of geo_scene.hip / geo_reg.hip.  A tile is 256 consecutive nodes (x fastest);
// a cell has the index of its lowest node, so the cell passes run over the same tiles.
//
//   mvster_tsdf_integrate       tsdf_integrate_kernel   one lane per node, a wave is a run along x; the loop over ALL views runs
//                                                       inside the lane with the view matrices read at wave-uniform addresses,
//                                                       the sums stay in registers, every output is written once
//   mvster_mesh_count           mesh_nodes_kernel       edge_mask [n] (7 bits), rank [n] = the node's vertices before it in its
//                                                       tile (uint16), vcounts [tile]
//                               mesh_cells_kernel       tcounts [tile] = the triangles of the tile's valid cells
//                               (mv_scan_counts) x 2    voffsets / toffsets [tiles + 1]: their last words are the vertex and the
//                                                       triangle count, the ONE read-back of an extraction
//   mvster_mesh_emit_vertices   mesh_vertices_kernel    vertex (A, d) goes to voffsets[tile] + rank[A] + popcount(mask below d)
//   mvster_mesh_emit_triangles  mesh_triangles_kernel   a cell ranks itself in its tile (wave scan + the tile's offset) and
//                                                       looks every corner's vertex up through its owner
// No atomics at all: two runs give the same bytes.
#include "common.hpp"
#include "tsdf_math.h"

namespace {

constexpr int kWG = 256;

struct IntegrateArgs {
    const float* depth;               // [V, H, W]
    const unsigned char* mask;        // [V, H, W]
    const unsigned char* images;      // [V, H, W, 3]
    const double* views;              // [V, 21]
    float* tsdf;                      // [nodes]
    int* weight;
    unsigned char* rgb;               // [nodes, 3]
    unsigned char* has_color;
    tsdf::Grid g;
    double trunc;
    long nodes;
    int V, H, W;
};

__global__ void __launch_bounds__(kWG) tsdf_integrate_kernel(IntegrateArgs a) {
    const long n = (long)blockIdx.x * kWG + threadIdx.x;
    if (n >= a.nodes) return;
    int i, j, k;
    tsdf::node_ijk(a.g, n, i, j, k);
    const double x = tsdf::coord(a.g.ox, a.g.voxel, i), y = tsdf::coord(a.g.oy, a.g.voxel, j), z = tsdf::coord(a.g.oz, a.g.voxel, k);
    const long hw = (long)a.H * a.W;
    tsdf::Sums s = tsdf::sums_empty();
    for (int v = 0; v < a.V; ++v)                                               // v is uniform: the matrices are scalar loads
        tsdf::add_view(a.views + (long)v * tsdf::kView, a.depth + v * hw, a.mask + v * hw, a.images + v * hw * 3, a.H, a.W, x, y, z,
                       a.trunc, s);
    a.tsdf[n] = tsdf::tsdf_of(s);
    a.weight[n] = s.w;
    a.rgb[n * 3 + 0] = tsdf::mean_byte(s.r, s.c);
    a.rgb[n * 3 + 1] = tsdf::mean_byte(s.g, s.c);
    a.rgb[n * 3 + 2] = tsdf::mean_byte(s.b, s.c);
    a.has_color[n] = s.c > 0 ? 1 : 0;
}

// the exclusive prefix of c over the workgroup's lanes in lane order, and the workgroup's total (every lane calls this)
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

struct MeshArgs {
    const float* tsdf;
    const int* weight;
    const unsigned char* rgb;
    const unsigned char* has_color;
    unsigned char* edge_mask;         // [nodes]
    unsigned short* rank;             // [nodes]
    int* vcounts;                     // [tiles]
    int* tcounts;                     // [tiles]
    const long* voffsets;             // [tiles + 1]
    const long* toffsets;             // [tiles + 1]
    float* vertices;                  // [Nv, 3]
    unsigned char* colors;            // [Nv, 3]
    int* triangles;                   // [Nt, 3]
    tsdf::Grid g;
    long nodes, Nv, Nt;
    int min_weight;
};

__global__ void __launch_bounds__(kWG) mesh_nodes_kernel(MeshArgs a) {
    __shared__ int wave_total[kWG / 64];
    const long n = (long)blockIdx.x * kWG + threadIdx.x;
    unsigned m = 0u;
    if (n < a.nodes) {
        int i, j, k;
        tsdf::node_ijk(a.g, n, i, j, k);
        m = tsdf::edge_mask(a.g, a.tsdf, a.weight, a.min_weight, i, j, k);
    }
    int total;
    const int before = tile_prefix(tsdf::popcount8(m), wave_total, total);
    if (n < a.nodes) {
        a.edge_mask[n] = (unsigned char)m;
        a.rank[n] = (unsigned short)before;                                     // < 256 * 7
    }
    if (threadIdx.x == 0) a.vcounts[blockIdx.x] = total;
}

__device__ __forceinline__ int cell_count(const MeshArgs& a, long n, unsigned& in) {
    in = 0u;
    if (n >= a.nodes) return 0;
    int i, j, k;
    tsdf::node_ijk(a.g, n, i, j, k);
    if (!tsdf::cell_valid(a.g, a.weight, a.min_weight, i, j, k)) return 0;
    in = tsdf::cell_inside(a.g, a.tsdf, n);
    return tsdf::cell_triangles(in);
}

__global__ void __launch_bounds__(kWG) mesh_cells_kernel(MeshArgs a) {
    __shared__ int wave_total[kWG / 64];
    unsigned in;
    int total;
    tile_prefix(cell_count(a, (long)blockIdx.x * kWG + threadIdx.x, in), wave_total, total);
    if (threadIdx.x == 0) a.tcounts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kWG) mesh_vertices_kernel(MeshArgs a) {
    const long n = (long)blockIdx.x * kWG + threadIdx.x;
    if (n >= a.nodes) return;
    const unsigned m = a.edge_mask[n];
    if (!m) return;
    int i, j, k;
    tsdf::node_ijk(a.g, n, i, j, k);
    const long base = a.voffsets[blockIdx.x] + a.rank[n];
    for (unsigned d = 1; d < 8u; ++d) {
        if (!((m >> d) & 1u)) continue;
        const long r = base + tsdf::edge_rank(m, d);
        if ((unsigned long)r >= (unsigned long)a.Nv) continue;                  // capacity of the caller's buffers
        float pos[3];
        unsigned char col[3];
        tsdf::vertex(a.g, a.tsdf, a.rgb, a.has_color, i, j, k, d, pos, col);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.vertices[r * 3 + c] = pos[c];
            a.colors[r * 3 + c] = col[c];
        }
    }
}

__global__ void __launch_bounds__(kWG) mesh_triangles_kernel(MeshArgs a) {
    __shared__ int wave_total[kWG / 64];
    const long n = (long)blockIdx.x * kWG + threadIdx.x;
    unsigned in;
    int total;
    const int count = cell_count(a, n, in);
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
                const long owner = n + tsdf::offset_index(a.g, lo);             // a corner of a valid cell: inside the grid
                a.triangles[r * 3 + c] = (int)(a.voffsets[owner / kWG] + a.rank[owner] + tsdf::edge_rank(a.edge_mask[owner], d));
            }
        }
    }
}

long tiles_of(long n) { return (n + kWG - 1) / kWG; }

bool grid_of(int nx, int ny, int nz, double ox, double oy, double oz, double voxel, tsdf::Grid& g) {
    if (!tsdf::grid_ok(nx, ny, nz)) return false;
    if (!(voxel > 0.0) || !(voxel < __builtin_huge_val()) || !(ox - ox == 0.0) || !(oy - oy == 0.0) || !(oz - oz == 0.0)) return false;
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.ox = ox; g.oy = oy; g.oz = oz; g.voxel = voxel;
    return true;
}

}  // namespace

extern "C" int mvster_mesh_blocks(long nodes) {
    if (nodes < 8 || nodes > tsdf::kMaxNodes) return MVSTER_ERR_SHAPE;
    return (int)tiles_of(nodes);
}

extern "C" int mvster_tsdf_integrate(const float* depth, const unsigned char* mask, const unsigned char* images, const double* views,
                                     int V, int H, int W, double ox, double oy, double oz, double voxel, int nx, int ny, int nz,
                                     double trunc, float* tsdf_out, int* weight, unsigned char* rgb, unsigned char* has_color,
                                     void* stream) {
    if (!depth || !mask || !images || !views || !tsdf_out || !weight || !rgb || !has_color) return MVSTER_ERR_NULL;
    IntegrateArgs a;
    if (!grid_of(nx, ny, nz, ox, oy, oz, voxel, a.g)) return MVSTER_ERR_SHAPE;
    if (V < 1 || H < 1 || W < 1 || H > tsdf::kMaxSide || W > tsdf::kMaxSide || !(trunc > 0.0) || !(trunc < __builtin_huge_val()))
        return MVSTER_ERR_SHAPE;
    a.depth = depth; a.mask = mask; a.images = images; a.views = views;
    a.tsdf = tsdf_out; a.weight = weight; a.rgb = rgb; a.has_color = has_color;
    a.trunc = trunc;
    a.nodes = tsdf::nodes_of(a.g);
    a.V = V; a.H = H; a.W = W;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)tiles_of(a.nodes)), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}

extern "C" int mvster_mesh_count(const float* tsdf_in, const int* weight, int nx, int ny, int nz, int min_weight,
                                 unsigned char* edge_mask, unsigned short* rank, int* vcounts, int* tcounts, long* voffsets,
                                 long* toffsets, void* stream) {
    if (!tsdf_in || !weight || !edge_mask || !rank || !vcounts || !tcounts || !voffsets || !toffsets) return MVSTER_ERR_NULL;
    MeshArgs a = {};
    if (!grid_of(nx, ny, nz, 0.0, 0.0, 0.0, 1.0, a.g)) return MVSTER_ERR_SHAPE;
    a.tsdf = tsdf_in; a.weight = weight; a.edge_mask = edge_mask; a.rank = rank; a.vcounts = vcounts; a.tcounts = tcounts;
    a.nodes = tsdf::nodes_of(a.g);
    a.min_weight = min_weight;
    const long tiles = tiles_of(a.nodes);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_nodes_kernel, dim3((unsigned)tiles), dim3(kWG), 0, st, a);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(mesh_cells_kernel, dim3((unsigned)tiles), dim3(kWG), 0, st, a);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    rc = mv_scan_counts(vcounts, voffsets, tiles, st);
    if (rc != MVSTER_OK) return rc;
    return mv_scan_counts(tcounts, toffsets, tiles, st);
}

extern "C" int mvster_mesh_emit_vertices(const float* tsdf_in, const unsigned char* rgb, const unsigned char* has_color, double ox,
                                         double oy, double oz, double voxel, int nx, int ny, int nz, const unsigned char* edge_mask,
                                         const unsigned short* rank, const long* voffsets, long Nv, float* vertices,
                                         unsigned char* colors, void* stream) {
    if (!tsdf_in || !rgb || !has_color || !edge_mask || !rank || !voffsets) return MVSTER_ERR_NULL;
    MeshArgs a = {};
    if (!grid_of(nx, ny, nz, ox, oy, oz, voxel, a.g) || Nv < 0 || Nv > 0x7fffffffl) return MVSTER_ERR_SHAPE;
    if (Nv == 0) return MVSTER_OK;                                              // no vertex: nothing to write
    if (!vertices || !colors) return MVSTER_ERR_NULL;
    a.tsdf = tsdf_in; a.rgb = rgb; a.has_color = has_color; a.edge_mask = const_cast<unsigned char*>(edge_mask);
    a.rank = const_cast<unsigned short*>(rank); a.voffsets = voffsets; a.vertices = vertices; a.colors = colors;
    a.nodes = tsdf::nodes_of(a.g);
    a.Nv = Nv;
    hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)tiles_of(a.nodes)), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}

extern "C" int mvster_mesh_emit_triangles(const float* tsdf_in, const int* weight, int nx, int ny, int nz, int min_weight,
                                          const unsigned char* edge_mask, const unsigned short* rank, const long* voffsets,
                                          const long* toffsets, long Nv, long Nt, int* triangles, void* stream) {
    if (!tsdf_in || !weight || !edge_mask || !rank || !voffsets || !toffsets) return MVSTER_ERR_NULL;
    MeshArgs a = {};
    if (!grid_of(nx, ny, nz, 0.0, 0.0, 0.0, 1.0, a.g) || Nv < 0 || Nv > 0x7fffffffl || Nt < 0) return MVSTER_ERR_SHAPE;
    if (Nt == 0) return MVSTER_OK;
    if (!triangles) return MVSTER_ERR_NULL;
    a.tsdf = tsdf_in; a.weight = weight; a.edge_mask = const_cast<unsigned char*>(edge_mask);
    a.rank = const_cast<unsigned short*>(rank); a.voffsets = voffsets; a.toffsets = toffsets; a.triangles = triangles;
    a.nodes = tsdf::nodes_of(a.g);
    a.Nv = Nv; a.Nt = Nt;
    a.min_weight = min_weight;
    hipLaunchKernelGGL(mesh_triangles_kernel, dim3((unsigned)tiles_of(a.nodes)), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}
