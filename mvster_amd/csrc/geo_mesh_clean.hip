// Cleaning an extracted mesh on the GPU (the definition is mesh_math.h): weld, degenerate triangles,
// connected components, their selection, compaction, and area-weighted vertex normals.  One lane per vertex or per triangle
// everywhere; integer atomics only, and every sum of floating-point numbers has a fixed order: two runs give the same bytes.
//
//   mvster_mesh_clean_plan
//     clean_table_kernel     (weld) claim [slots] = -1, first [slots] = INT_MAX
//     clean_init_kernel      parent[v] = v, used = counts = 0, canon[v] = v, the statistics and the best key = 0
//     clean_insert_kernel    (weld) one lane per finite vertex: claim-or-find its slot in the open-addressing table (a slot is
//                            claimed by compare-and-swap of the vertex's INDEX, a collision is told from a match by comparing
//                            the claimant's position, which is read-only input), atomicMin of the index on first[slot]
//     clean_canon_kernel     (weld) canon[v] = first[slot of v]: final, since the launch before is over
//     clean_hook_kernel      one lane per triangle: canonical corners, dropped or kept, used[], and two unions in the lock-free
//                            union-find (below)
//     clean_flatten_kernel   labels[v] = the root of v, -1 for an unused or welded-away vertex: a launch of its own, so parent[]
//                            is read-only here and plain loads see all of the hooking launch
//     clean_count_kernel     vertices and triangles per root (integer atomics, a run of lanes with one root adds once), the
//                            root flags and the roots per workgroup
//     (mv_scan_counts)       over the workgroups' root counts (section 4.10's single-workgroup scan)
//     clean_table_rows_kernel  a root ranks itself (the flags before it in its workgroup + the workgroup's offset), writes its
//                            row of the table and offers size_key to one 64-bit atomicMax
//     clean_keep_kernel      component kept? -> the triangle and vertex flags and their number per workgroup, tri_component
//     (mv_scan_counts) x 2   over the workgroups' kept vertices / triangles
//     clean_number_kernel    every kept vertex and triangle gets its new number the same way; Nv', Nt' and the number of
//                            components go beside the statistics: the caller's ONE read-back
//   mvster_mesh_clean_emit
//     clean_emit_kernel      a kept vertex / triangle writes itself at its number
//   mvster_mesh_vertex_normals
//     normals_zero_kernel, normals_valence_kernel   corners per vertex (integer atomics)
//     normals_local_kernel   a vertex's corners before it in its workgroup, the workgroup's corners
//     (mv_scan_counts)       over the workgroups: a row starts at its workgroup's offset + the corners before it there
//     normals_fill_kernel    every corner takes a place in its vertex's row with an atomic decrement: the order inside a row
//                            depends on the schedule ...
//     normals_sum_kernel     ... so the row's lane first puts it into ascending order (mesh::sort_row), then sums in that order
//
// Union-find.  parent[x] <= x always: a root is only ever linked under a SMALLER root (compare-and-swap of parent[r] from r),
// and the one other write, atomicMin(parent[x], y), is made with a y < x found in x's own tree; trees only ever merge, so it
// keeps the forest and its sets.  So chains strictly decrease, a component's final root is its smallest vertex whatever the
// interleaving, and nothing ever waits for another lane.  Inside the hooking launch every access to parent[] is an agent-scope
// atomic (load, min, compare-and-swap): a plain load could be served from this CU's L1 or another XCD's L2 and miss a link.
#include <limits.h>

#include "common.hpp"
#include "mesh_math.h"

namespace {

constexpr int kWG = 256;

// the statistics the host reads back in one copy (longs)
enum { kStatVertices = 0, kStatTriangles, kStatComponents, kStatCanonical, kStatDropped, kStatKept, kStatStatus, kStatBest, kStats };

struct CleanArgs {
    const float* vertices;            // [Nv, 3]; NULL: no position is looked at (components of an index list)
    const int* triangles;             // [Nt, 3]
    long Nv, Nt;
    int* claim;                       // [slots] the vertex that claimed the slot, -1 = free
    int* first;                       // [slots] the smallest vertex of the slot
    unsigned mask;                    // slots - 1
    int* canon;                       // [Nv]
    int* parent;                      // [Nv]
    int* used;                        // [Nv]
    int* cnt_v;                       // [Nv] vertices per root
    int* cnt_t;                       // [Nv] triangles per root
    int* root_flag;                   // [Nv]
    int* root_rank;                   // [Nv] a root's row in the component table
    int* vkeep;                       // [Nv]
    int* vnum;                        // [Nv] a kept vertex's new number
    int* tkeep;                       // [Nt]
    int* tnum;                        // [Nt] a kept triangle's new number
    int* wg_roots;                    // [blocks] per workgroup of 256: roots, kept vertices, kept triangles
    int* wg_vkeep;
    int* wg_tkeep;
    int* labels;                      // [Nv]
    int* tri_labels;                  // [Nt]
    int* tri_component;               // [Nt]
    int* roots;                       // [ccap]
    int* comp_vertices;               // [ccap]
    int* comp_triangles;              // [ccap]
    long ccap;
    long* roff;                       // [blocks + 1] the exclusive scans of the three
    long* voff;
    long* toff;
    long blocks;                      // workgroups of 256 over max(Nv, Nt)
    unsigned long long* stats;        // [kStats]
    long min_triangles;
    int largest_only;
};

__global__ void __launch_bounds__(kWG) clean_table_kernel(int* __restrict__ claim, int* __restrict__ first, long slots) {
    const long s = (long)blockIdx.x * kWG + threadIdx.x;
    if (s < slots) {
        claim[s] = -1;
        first[s] = INT_MAX;
    }
}

__global__ void __launch_bounds__(kWG) clean_init_kernel(CleanArgs a) {
    const long v = (long)blockIdx.x * kWG + threadIdx.x;
    if (v < kStats) a.stats[v] = 0ull;
    if (v >= a.Nv) return;
    a.canon[v] = (int)v;
    a.parent[v] = (int)v;
    a.used[v] = 0;
    a.cnt_v[v] = 0;
    a.cnt_t[v] = 0;
}

// the lanes of the wave with `flag` are added to *word by the wave's first lane (every lane of the wave calls this)
__device__ __forceinline__ void wave_add(bool flag, unsigned long long* word) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(word, (unsigned long long)__popcll(b));
}

// The lanes of the workgroup with `flag` before this one in lane order, and their number in the workgroup (every lane calls
// this).  wave_count: kWG / 64 ints of LDS, one use per call site.
__device__ __forceinline__ int flags_before(bool flag, int* wave_count, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wave_count[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int w = 0; w < kWG / 64; ++w) {
        if (w < wave) before += wave_count[w];
        total += wave_count[w];
    }
    return before;
}

__global__ void __launch_bounds__(kWG) clean_insert_kernel(CleanArgs a) {
    const long v = (long)blockIdx.x * kWG + threadIdx.x;
    if (v >= a.Nv) return;
    const float* p = a.vertices + 3 * v;
    if (!mesh::finite3(p)) return;                                              // coincides with nothing: canon[v] stays v
    int found = -1;
    unsigned s = (unsigned)mesh::position_hash(p) & a.mask;
    for (unsigned it = 0; it <= a.mask; ++it) {                                 // ends: at most `slots` probes, no waiting
        int cur = __hip_atomic_load(&a.claim[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur < 0) {
            cur = atomicCAS(&a.claim[s], -1, (int)v);
            if (cur < 0) cur = (int)v;                                          // claimed
        }
        if (mesh::index_ok(cur, a.Nv) && mesh::same_position(a.vertices + 3l * cur, p)) {
            found = (int)s;
            break;
        }
        s = (s + 1) & a.mask;
    }
    if (found >= 0) {
        atomicMin(&a.first[found], (int)v);
        a.canon[v] = -2 - found;                                                // the slot, until clean_canon_kernel
    } else {
        a.stats[kStatStatus] = 1ull;                                            // table full: the host turns this into an error
    }
}

__global__ void __launch_bounds__(kWG) clean_canon_kernel(CleanArgs a) {
    const long v = (long)blockIdx.x * kWG + threadIdx.x;
    bool canonical = false;
    if (v < a.Nv) {
        int c = a.canon[v];
        if (c <= -2) {
            c = a.first[-2 - c];
            if (!mesh::index_ok(c, a.Nv)) c = (int)v;
            a.canon[v] = c;
        }
        canonical = c == (int)v;
    }
    wave_add(canonical, &a.stats[kStatCanonical]);
}

__device__ __forceinline__ int uf_load(int* parent, int x) {
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x at some moment of the launch.  Ends: parent[y] < y for every y that is not a root, so y strictly decreases
// and is bounded by 0; no step waits for anybody.
__device__ __forceinline__ int uf_find(int* parent, int x) {
    int y = x;
    for (int p = uf_load(parent, y); p != y; p = uf_load(parent, y)) y = p;
    if (y != x) atomicMin(&parent[x], y);                                       // a shortcut: y < x is in x's tree; trees only merge
    return y;
}

// Ends: each pass either finds one root (done), links the larger root under the smaller by its own compare-and-swap (done),
// or its compare-and-swap failed because another lane's succeeded on x, after which the root found from x is strictly smaller
// than x: x + y strictly decreases from pass to pass and is bounded by 0.  A failure always means somebody else's progress.
__device__ __forceinline__ void uf_unite(int* parent, int x, int y) {
    for (;;) {
        x = uf_find(parent, x);
        y = uf_find(parent, y);
        if (x == y) return;
        if (x < y) {
            const int t = x;
            x = y;
            y = t;
        }
        if (atomicCAS(&parent[x], x, y) == x) return;                           // x was still a root: now under the smaller y
    }
}

__global__ void __launch_bounds__(kWG) clean_hook_kernel(CleanArgs a) {
    const long t = (long)blockIdx.x * kWG + threadIdx.x;
    bool dropped = false;
    if (t < a.Nt) {
        int c[3];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = a.triangles[3 * t + k];
            ok = ok && mesh::index_ok(c[k], a.Nv);                              // (the caller refuses such a mesh)
            c[k] = ok ? a.canon[c[k]] : 0;
        }
        dropped = !ok || mesh::triangle_dropped(a.vertices, c[0], c[1], c[2]);
        a.tri_labels[t] = dropped ? -1 : c[0];                                  // a corner, until clean_count_kernel
        if (!dropped) {
            a.used[c[0]] = 1;                                                   // (every writer writes 1; read in later launches)
            a.used[c[1]] = 1;
            a.used[c[2]] = 1;
            uf_unite(a.parent, c[0], c[1]);
            uf_unite(a.parent, c[0], c[2]);
        }
    }
    wave_add(dropped, &a.stats[kStatDropped]);
}

__global__ void __launch_bounds__(kWG) clean_flatten_kernel(CleanArgs a) {
    const long v = (long)blockIdx.x * kWG + threadIdx.x;
    if (v >= a.Nv) return;
    int label = -1;
    if (a.canon[v] == (int)v && a.used[v]) {
        label = (int)v;
        for (int p = a.parent[label]; p != label; p = a.parent[label]) label = p;   // ends: strictly decreasing, nobody writes
    }
    a.labels[v] = label;
}

// Every lane of the wave calls this; key < 0 adds nothing.  A run of consecutive lanes with one key adds its length once: a
// mesh in one piece would otherwise send every lane's atomic to one word.
__device__ __forceinline__ void add_runs(int* counts, int key) {
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1, 64);
    const bool starts = lane == 0 || prev != key;
    const unsigned long long sb = __ballot(starts);
    if (key < 0 || !starts) return;
    const unsigned long long above = lane == 63 ? 0ull : sb & ~((2ull << lane) - 1ull);
    const int next = above ? __ffsll((long long)above) - 1 : 64;
    atomicAdd(&counts[key], next - lane);
}

__global__ void __launch_bounds__(kWG) clean_count_kernel(CleanArgs a) {
    __shared__ int wave_count[kWG / 64];
    const long i = (long)blockIdx.x * kWG + threadIdx.x;
    int tl = -1, vl = -1;
    if (i < a.Nt) {
        const int corner = a.tri_labels[i];
        if (corner >= 0) tl = a.labels[corner];
        a.tri_labels[i] = tl;
    }
    if (i < a.Nv) {
        vl = a.labels[i];
        a.root_flag[i] = vl == (int)i ? 1 : 0;
    }
    add_runs(a.cnt_t, tl);
    add_runs(a.cnt_v, vl);
    int total;
    flags_before(i < a.Nv && vl == (int)i, wave_count, total);
    if (threadIdx.x == 0) a.wg_roots[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kWG) clean_table_rows_kernel(CleanArgs a) {
    __shared__ int wave_count[kWG / 64];
    const long v = (long)blockIdx.x * kWG + threadIdx.x;
    const bool root = v < a.Nv && a.root_flag[v];
    int total;
    const long r = a.roff[blockIdx.x] + flags_before(root, wave_count, total);
    if (!root) return;
    a.root_rank[v] = (int)r;
    if ((unsigned long)r < (unsigned long)a.ccap) {
        a.roots[r] = (int)v;
        a.comp_vertices[r] = a.cnt_v[v];
        a.comp_triangles[r] = a.cnt_t[v];
    }
    atomicMax(&a.stats[kStatBest], mesh::size_key(a.cnt_t[v], (int)v));
}

__global__ void __launch_bounds__(kWG) clean_keep_kernel(CleanArgs a) {
    __shared__ int wave_count[2][kWG / 64];
    const long i = (long)blockIdx.x * kWG + threadIdx.x;
    const unsigned long long best = a.stats[kStatBest];                         // final: written by the launch before
    const bool largest = a.largest_only != 0;
    bool tkeep = false, vkeep = false, kept_root = false;
    if (i < a.Nt) {
        const int l = a.tri_labels[i];
        a.tri_component[i] = l >= 0 ? a.root_rank[l] : -1;
        tkeep = l >= 0 && mesh::component_kept(a.cnt_t[l], l, a.min_triangles, largest, best);
        a.tkeep[i] = tkeep ? 1 : 0;
    }
    if (i < a.Nv) {
        const int l = a.labels[i];
        vkeep = l >= 0 && mesh::component_kept(a.cnt_t[l], l, a.min_triangles, largest, best);
        a.vkeep[i] = vkeep ? 1 : 0;
        kept_root = vkeep && l == (int)i;
    }
    wave_add(kept_root, &a.stats[kStatKept]);
    int vtotal, ttotal;
    flags_before(vkeep, wave_count[0], vtotal);
    flags_before(tkeep, wave_count[1], ttotal);
    if (threadIdx.x == 0) {
        a.wg_vkeep[blockIdx.x] = vtotal;
        a.wg_tkeep[blockIdx.x] = ttotal;
    }
}

__global__ void __launch_bounds__(kWG) clean_number_kernel(CleanArgs a) {
    __shared__ int wave_count[2][kWG / 64];
    const long i = (long)blockIdx.x * kWG + threadIdx.x;
    const bool vkeep = i < a.Nv && a.vkeep[i], tkeep = i < a.Nt && a.tkeep[i];
    int total;
    const long vn = a.voff[blockIdx.x] + flags_before(vkeep, wave_count[0], total);
    const long tn = a.toff[blockIdx.x] + flags_before(tkeep, wave_count[1], total);
    if (i < a.Nv) a.vnum[i] = vkeep ? (int)vn : -1;
    if (i < a.Nt) a.tnum[i] = tkeep ? (int)tn : -1;
    if (i == 0) {
        a.stats[kStatVertices] = (unsigned long long)a.voff[a.blocks];
        a.stats[kStatTriangles] = (unsigned long long)a.toff[a.blocks];
        a.stats[kStatComponents] = (unsigned long long)a.roff[a.blocks];
    }
}

struct EmitArgs {
    const float* vertices;
    const unsigned char* colors;      // may be NULL
    const int* triangles;
    const int* canon;
    const int* vnum;                  // [Nv] the new number, -1 = not kept
    const int* tnum;                  // [Nt]
    float* out_vertices;
    unsigned char* out_colors;
    int* out_triangles;
    long* vertex_index;
    long* triangle_index;
    long Nv, Nt, NvOut, NtOut;
};

__global__ void __launch_bounds__(kWG) clean_emit_kernel(EmitArgs a) {
    const long i = (long)blockIdx.x * kWG + threadIdx.x;
    if (i < a.Nv) {
        const long r = a.vnum[i];
        if ((unsigned long)r < (unsigned long)a.NvOut) {                        // kept, and within the caller's capacity
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a.out_vertices[3 * r + k] = a.vertices[3 * i + k];
                if (a.colors) a.out_colors[3 * r + k] = a.colors[3 * i + k];
            }
            a.vertex_index[r] = i;
        }
    }
    if (i < a.Nt) {
        const long r = a.tnum[i];
        if ((unsigned long)r < (unsigned long)a.NtOut) {
#pragma unroll
            for (int k = 0; k < 3; ++k)                                         // (a kept triangle: its indices are in range)
                a.out_triangles[3 * r + k] = a.vnum[a.canon[a.triangles[3 * i + k]]];
            a.triangle_index[r] = i;
        }
    }
}

// ---- vertex normals -------------------------------------------------------------------------------------------------------------

struct NormalArgs {
    const float* vertices;            // [Nv, 3]
    const int* triangles;             // [Nt, 3]
    int* counts;                      // [Nv] corners per vertex; the fill pass counts it back down to 0
    int* local;                       // [Nv] the corners of the vertices before this one in its workgroup
    int* wg_counts;                   // [blocks] corners per workgroup
    long* wg_offsets;                 // [blocks + 1] their exclusive scan
    int* rows;                        // [3 Nt] triangle numbers, a row per vertex
    float* normals;                   // [Nv, 3]
    unsigned char* valid;             // [Nv]
    long Nv, Nt;
};

__global__ void __launch_bounds__(kWG) normals_zero_kernel(NormalArgs a) {
    const long v = (long)blockIdx.x * kWG + threadIdx.x;
    if (v < a.Nv) a.counts[v] = 0;
}

// a triangle with an index outside 0 .. Nv-1 takes no part (the caller refuses such a mesh; never out of bounds)
__device__ __forceinline__ bool corners_of(const NormalArgs& a, long t, int c[3]) {
    if (t >= a.Nt) return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = a.triangles[3 * t + k];
        ok = ok && mesh::index_ok(c[k], a.Nv);
    }
    return ok;
}

__global__ void __launch_bounds__(kWG) normals_valence_kernel(NormalArgs a) {
    int c[3];
    const bool ok = corners_of(a, (long)blockIdx.x * kWG + threadIdx.x, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) add_runs(a.counts, ok ? c[k] : -1);             // (a fan's hub: one add per wave, not per lane)
}

__global__ void __launch_bounds__(kWG) normals_local_kernel(NormalArgs a) {
    __shared__ int wave_total[kWG / 64];
    const long v = (long)blockIdx.x * kWG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = v < a.Nv ? a.counts[v] : 0;
    int x = c;                                                                  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wave_total[wave] = x;
    __syncthreads();
    int before = x - c, total = 0;
#pragma unroll
    for (int w = 0; w < kWG / 64; ++w) {
        if (w < wave) before += wave_total[w];
        total += wave_total[w];
    }
    if (v < a.Nv) a.local[v] = before;
    if (threadIdx.x == 0) a.wg_counts[blockIdx.x] = total;
}

// where vertex v's row starts (v = Nv: where the last row ends)
__device__ __forceinline__ long row_begin(const NormalArgs& a, long v) {
    return v < a.Nv ? a.wg_offsets[v / kWG] + a.local[v] : a.wg_offsets[(a.Nv + kWG - 1) / kWG];
}

__global__ void __launch_bounds__(kWG) normals_fill_kernel(NormalArgs a) {
    const long t = (long)blockIdx.x * kWG + threadIdx.x;
    int c[3];
    if (!corners_of(a, t, c)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int place = atomicSub(&a.counts[c[k]], 1) - 1;                    // 0 .. valence - 1, each once
        if (place >= 0) a.rows[row_begin(a, c[k]) + place] = (int)t;
    }
}

__global__ void __launch_bounds__(kWG) normals_sum_kernel(NormalArgs a) {
    const long v = (long)blockIdx.x * kWG + threadIdx.x;
    if (v >= a.Nv) return;
    const long begin = row_begin(a, v), L = row_begin(a, v + 1) - begin;
    int* row = a.rows + begin;                                                  // this lane's own: nobody else touches it here
    mesh::sort_row(row, L);
    double N[3] = {0.0, 0.0, 0.0};
    for (long k = 0; k < L; ++k) {
        const int* c = a.triangles + 3l * row[k];
        double n[3];
        mesh::triangle_normal(a.vertices + 3l * c[0], a.vertices + 3l * c[1], a.vertices + 3l * c[2], n);
        N[0] = N[0] + n[0];
        N[1] = N[1] + n[1];
        N[2] = N[2] + n[2];
    }
    float out[3];
    a.valid[v] = mesh::unit_normal(N, out) ? 1 : 0;
    a.normals[3 * v + 0] = out[0];
    a.normals[3 * v + 1] = out[1];
    a.normals[3 * v + 2] = out[2];
}

unsigned blocks_of(long n) { return (unsigned)((n + kWG - 1) / kWG); }

bool sizes_ok(long Nv, long Nt) { return Nv >= 0 && Nv <= mesh::kMaxVertices && Nt >= 0 && Nt <= mesh::kMaxTriangles; }

#define MV_LAUNCH(kernel, n, ...)                                                                  \
    do {                                                                                           \
        hipLaunchKernelGGL(kernel, dim3(blocks_of(n)), dim3(kWG), 0, st, __VA_ARGS__);             \
        const int rc_ = mv_check_launch();                                                         \
        if (rc_ != MVSTER_OK) return rc_;                                                          \
    } while (0)

}  // namespace

extern "C" int mvster_mesh_clean_work(long Nv, long Nt, long* work_ints, long* work_longs) {
    if (!work_ints || !work_longs) return MVSTER_ERR_NULL;
    if (!sizes_ok(Nv, Nt)) return MVSTER_ERR_SHAPE;
    const long blocks = (long)blocks_of(Nv > Nt ? Nv : Nt);
    *work_ints = 8 * Nv + 2 * Nt + 3 * blocks;
    *work_longs = 3 * (blocks + 1) + kStats;
    return MVSTER_OK;
}

extern "C" int mvster_mesh_normals_blocks(long Nv) {
    if (!sizes_ok(Nv, 0)) return MVSTER_ERR_SHAPE;
    return (int)blocks_of(Nv);
}

extern "C" int mvster_mesh_clean_plan(const float* vertices, const int* triangles, long Nv, long Nt, int weld, long min_triangles,
                                      int largest_only, int* table, long table_slots, int* canon, int* labels, int* tri_labels,
                                      int* tri_component, int* roots, int* comp_vertices, int* comp_triangles, long component_rows,
                                      int* work_ints, long* work_longs, void* stream) {
    if (!triangles || !canon || !labels || !tri_labels || !tri_component || !roots || !comp_vertices || !comp_triangles ||
        !work_ints || !work_longs)
        return MVSTER_ERR_NULL;
    if (weld && (!vertices || !table)) return MVSTER_ERR_NULL;
    if (!sizes_ok(Nv, Nt) || min_triangles < 0 || component_rows < 0 || (weld != 0 && weld != 1) ||
        (largest_only != 0 && largest_only != 1))
        return MVSTER_ERR_SHAPE;
    if (weld && !mesh::slots_ok(table_slots, Nv)) return MVSTER_ERR_SHAPE;
    if (Nv == 0 || Nt == 0) return MVSTER_OK;                                   // an empty mesh: nothing to launch
    CleanArgs a = {};
    a.vertices = vertices; a.triangles = triangles; a.Nv = Nv; a.Nt = Nt;
    a.claim = table; a.first = weld ? table + table_slots : nullptr; a.mask = weld ? (unsigned)(table_slots - 1) : 0u;
    a.canon = canon; a.labels = labels; a.tri_labels = tri_labels; a.tri_component = tri_component;
    a.roots = roots; a.comp_vertices = comp_vertices; a.comp_triangles = comp_triangles; a.ccap = component_rows;
    const long both = Nv > Nt ? Nv : Nt, blocks = (long)blocks_of(both);
    a.parent = work_ints; a.used = work_ints + Nv; a.cnt_v = work_ints + 2 * Nv; a.cnt_t = work_ints + 3 * Nv;
    a.root_flag = work_ints + 4 * Nv; a.root_rank = work_ints + 5 * Nv; a.vkeep = work_ints + 6 * Nv; a.vnum = work_ints + 7 * Nv;
    a.tkeep = work_ints + 8 * Nv; a.tnum = a.tkeep + Nt;
    a.wg_roots = a.tnum + Nt; a.wg_vkeep = a.wg_roots + blocks; a.wg_tkeep = a.wg_vkeep + blocks;
    a.roff = work_longs; a.voff = work_longs + (blocks + 1); a.toff = work_longs + 2 * (blocks + 1);
    a.stats = reinterpret_cast<unsigned long long*>(work_longs + 3 * (blocks + 1));
    a.blocks = blocks;
    a.min_triangles = min_triangles; a.largest_only = largest_only;
    hipStream_t st = (hipStream_t)stream;
    if (weld) MV_LAUNCH(clean_table_kernel, table_slots, a.claim, a.first, table_slots);
    MV_LAUNCH(clean_init_kernel, Nv > kStats ? Nv : (long)kStats, a);
    if (weld) MV_LAUNCH(clean_insert_kernel, Nv, a);
    MV_LAUNCH(clean_canon_kernel, Nv, a);
    MV_LAUNCH(clean_hook_kernel, Nt, a);
    MV_LAUNCH(clean_flatten_kernel, Nv, a);
    MV_LAUNCH(clean_count_kernel, both, a);
    int rc = mv_scan_counts(a.wg_roots, a.roff, blocks, st);
    if (rc != MVSTER_OK) return rc;
    MV_LAUNCH(clean_table_rows_kernel, both, a);                                // (the count pass's grid: the offsets are per its workgroups)
    MV_LAUNCH(clean_keep_kernel, both, a);
    rc = mv_scan_counts(a.wg_vkeep, a.voff, blocks, st);
    if (rc != MVSTER_OK) return rc;
    rc = mv_scan_counts(a.wg_tkeep, a.toff, blocks, st);
    if (rc != MVSTER_OK) return rc;
    MV_LAUNCH(clean_number_kernel, both, a);
    return MVSTER_OK;
}

extern "C" int mvster_mesh_clean_emit(const float* vertices, const unsigned char* colors, const int* triangles, long Nv, long Nt,
                                      const int* canon, const int* work_ints, long NvOut, long NtOut,
                                      float* out_vertices, unsigned char* out_colors, int* out_triangles, long* vertex_index,
                                      long* triangle_index, void* stream) {
    if (!vertices || !triangles || !canon || !work_ints) return MVSTER_ERR_NULL;
    if (!sizes_ok(Nv, Nt) || NvOut < 0 || NvOut > Nv || NtOut < 0 || NtOut > Nt) return MVSTER_ERR_SHAPE;
    if (NvOut == 0 && NtOut == 0) return MVSTER_OK;                             // nothing kept: nothing to write
    if ((NvOut > 0 && (!out_vertices || !vertex_index || (colors && !out_colors))) ||
        (NtOut > 0 && (!out_triangles || !triangle_index)))
        return MVSTER_ERR_NULL;
    EmitArgs a = {};
    a.vertices = vertices; a.colors = colors; a.triangles = triangles; a.canon = canon;
    a.vnum = work_ints + 7 * Nv; a.tnum = work_ints + 8 * Nv + Nt;
    a.out_vertices = out_vertices; a.out_colors = out_colors; a.out_triangles = out_triangles;
    a.vertex_index = vertex_index; a.triangle_index = triangle_index;
    a.Nv = Nv; a.Nt = Nt; a.NvOut = NvOut; a.NtOut = NtOut;
    hipStream_t st = (hipStream_t)stream;
    MV_LAUNCH(clean_emit_kernel, Nv > Nt ? Nv : Nt, a);
    return MVSTER_OK;
}

extern "C" int mvster_mesh_vertex_normals(const float* vertices, const int* triangles, long Nv, long Nt, int* work_ints,
                                          long* work_longs, int* rows, float* normals, unsigned char* valid, void* stream) {
    if (!sizes_ok(Nv, Nt)) return MVSTER_ERR_SHAPE;
    if (Nv == 0) return MVSTER_OK;                                              // no vertex: nothing to write
    if (!vertices || !work_ints || !work_longs || !normals || !valid || (Nt > 0 && (!triangles || !rows))) return MVSTER_ERR_NULL;
    NormalArgs a = {};
    const long blocks = (long)blocks_of(Nv);
    a.vertices = vertices; a.triangles = triangles; a.counts = work_ints; a.local = work_ints + Nv; a.wg_counts = work_ints + 2 * Nv;
    a.wg_offsets = work_longs; a.rows = rows;
    a.normals = normals; a.valid = valid; a.Nv = Nv; a.Nt = Nt;
    hipStream_t st = (hipStream_t)stream;
    MV_LAUNCH(normals_zero_kernel, Nv, a);
    if (Nt > 0) MV_LAUNCH(normals_valence_kernel, Nt, a);
    MV_LAUNCH(normals_local_kernel, Nv, a);
    const int rc = mv_scan_counts(a.wg_counts, a.wg_offsets, blocks, st);
    if (rc != MVSTER_OK) return rc;
    if (Nt > 0) MV_LAUNCH(normals_fill_kernel, Nt, a);
    MV_LAUNCH(normals_sum_kernel, Nv, a);
    return MVSTER_OK;
}
