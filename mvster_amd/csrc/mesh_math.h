// Cleaning an extracted mesh: welding of coinciding vertices, removal of degenerate triangles,
// connected components and their selection, compaction, and area-weighted vertex normals -- the definition, shared by
// geo_mesh_clean.hip and the host build used only by the tests (tests/hostmath/mesh_clean_hostmath.cpp).  Like tsdf_math.h:
// IEEE fp64, one correctly rounded operation per step in the order written, only + - * / sqrt, contraction switched off for
// both compilers, and no call into libm, so the kernels and the host build give the same bits.  It is this project's own
// definition; DESIGN.md lists the deviations from Open3D.
//
// A mesh is vertices [Nv,3] float32, triangles [Nt,3] int32 with every index in 0 .. Nv-1, and optionally colors [Nv,3] uint8.
//
// Weld.  Two vertices COINCIDE if all three coordinates compare equal as floats (so -0.0 equals +0.0); a vertex with a
// coordinate that is not finite coincides with nothing.  canon[v] = the smallest index among the vertices coinciding with v
// (v itself without welding).  A canonical vertex keeps its own position and colour bytes; nothing is averaged.
//
// Degenerate triangles.  With (a, b, c) = canon of its corners, a triangle is DROPPED if a == b, a == c or b == c, or if a
// corner has a coordinate that is not finite.  A triangle with three distinct collinear corners is kept (dropping it would
// leave a T-junction), and duplicate triangles are not looked for.
//
// Components.  Two kept triangles are connected if they share a canonical vertex (vertex connectivity; Open3D's
// cluster_connected_triangles uses shared edges).  label[v] = the smallest vertex index in v's component for a canonical vertex
// used by a kept triangle, -1 otherwise; a kept triangle's label is that of its corners, a dropped one's -1.  The component
// table lists the roots (the vertices with label[v] == v) ascending with the vertices and triangles of each, and
// tri_component[t] is the rank of the triangle's root in that table (-1 for a dropped triangle).
//
// Selection.  A component is kept iff n_triangles >= min_triangles and, with largest_only, it is THE component with the most
// triangles, ties going to the smaller root: the one whose size_key(n_triangles, root) is greatest.
//
// Compaction.  The triangles of kept components stay in input order; the vertices kept are the canonical vertices used by one of
// them, in input order; triangle indices are renumbered; vertex_index / triangle_index point into the input.
//
// Vertex normals.  For triangle t with corners a, b, c: the float32 positions widened to fp64, e1 = b - a, e2 = c - a,
//   n_t = (e1.y e2.z - e1.z e2.y,  e1.z e2.x - e1.x e2.z,  e1.x e2.y - e1.y e2.x)
// (twice the area times the unit normal, counter-clockwise seen from its tip).  N_v = the sum of n_t over the triangles that
// name v in ASCENDING TRIANGLE INDEX, per coordinate from left to right, a triangle that names v twice counting once per
// occurrence.  len = sqrt((N.x^2 + N.y^2) + N.z^2); normal = (float)(N / len) and valid = 1, or (0, 0, 0) and valid = 0 where
// len is 0 or not finite (an unused vertex included).  Open3D sums unit triangle normals instead.
#pragma once
#include "mvster_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace mesh {

constexpr long kMaxVertices = 1l << 29;           // the weld table holds at most 2^30 slots, at least 2 per vertex
constexpr long kMaxTriangles = 1l << 29;          // 3 Nt corners are counted in 32 bits
constexpr long kMinSlots = 64;
constexpr long kMaxSlots = 1l << 30;
constexpr int kInsertionRow = 16;                 // rows up to this length are put in order by insertion, longer ones by a heap

MV_HD bool finite32(float x) { return x - x == 0.0f; }
MV_HD bool finite3(const float* p) { return finite32(p[0]) && finite32(p[1]) && finite32(p[2]); }
MV_HD bool same_position(const float* a, const float* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

MV_HD bool slots_ok(long slots, long Nv) {
    return slots >= kMinSlots && slots <= kMaxSlots && !(slots & (slots - 1)) && slots >= 2 * Nv;
}

// the bits of a finite coordinate with -0.0 taken to +0.0: equal floats give equal words
MV_HD unsigned coord_bits(float x) {
    const float y = x == 0.0f ? 0.0f : x;
    unsigned u;
    __builtin_memcpy(&u, &y, 4);
    return u;
}

// where a position's probing starts (nothing computed depends on it but the time the table takes)
MV_HD unsigned long long position_hash(const float* p) {
    unsigned long long h = ((unsigned long long)coord_bits(p[0]) << 32 | coord_bits(p[1])) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h = (h + coord_bits(p[2])) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    h *= 0x94D049BB133111EBull;
    return h ^ (h >> 31);
}

MV_HD bool index_ok(int i, long Nv) { return (unsigned long)(long)i < (unsigned long)Nv; }

// (a, b, c): the canonical corners of a triangle; `vertices` may be NULL (no position is looked at then)
MV_HD bool triangle_dropped(const float* vertices, int a, int b, int c) {
    if (a == b || a == c || b == c) return true;
    if (!vertices) return false;
    return !finite3(vertices + 3l * a) || !finite3(vertices + 3l * b) || !finite3(vertices + 3l * c);
}

MV_HD unsigned long long size_key(int n_triangles, int root) {
    return (unsigned long long)(unsigned)n_triangles << 32 | (0xFFFFFFFFu - (unsigned)root);
}
MV_HD int key_root(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

// best: the greatest size_key over the components
MV_HD bool component_kept(int n_triangles, int root, long min_triangles, bool largest_only, unsigned long long best) {
    return (long)n_triangles >= min_triangles && (!largest_only || key_root(best) == root);
}

MV_HD void triangle_normal(const float* a, const float* b, const float* c, double n[3]) {
    const double e1x = (double)b[0] - (double)a[0], e1y = (double)b[1] - (double)a[1], e1z = (double)b[2] - (double)a[2];
    const double e2x = (double)c[0] - (double)a[0], e2y = (double)c[1] - (double)a[1], e2z = (double)c[2] - (double)a[2];
    n[0] = e1y * e2z - e1z * e2y;
    n[1] = e1z * e2x - e1x * e2z;
    n[2] = e1x * e2y - e1y * e2x;
}

// N: a vertex's sum -> its normal; false (and zeros) where the length is 0 or not finite
MV_HD bool unit_normal(const double N[3], float out[3]) {
    const double len = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
    if (!(len > 0.0) || !(len < __builtin_huge_val())) {
        out[0] = out[1] = out[2] = 0.0f;
        return false;
    }
    out[0] = (float)(N[0] / len);
    out[1] = (float)(N[1] / len);
    out[2] = (float)(N[2] / len);
    return true;
}

// a vertex's row of triangle numbers into ascending order, in place (equal numbers -- a triangle that names the vertex twice --
// stay next to each other; which of them comes first changes nothing).  Insertion for a short row; a heap for a long one, so
// the work is O(L log L) for any valence.
MV_HD void sort_row(int* row, long L) {
    if (L <= kInsertionRow) {
        for (long i = 1; i < L; ++i) {
            const int x = row[i];
            long j = i;
            for (; j > 0 && row[j - 1] > x; --j) row[j] = row[j - 1];
            row[j] = x;
        }
        return;
    }
    for (long start = L / 2, end = L; end > 1;) {                              // heapsort: build the max-heap, then pop
        if (start > 0) {
            --start;
        } else {
            --end;
            const int x = row[end];
            row[end] = row[0];
            row[0] = x;
        }
        long root = start;
        const int x = row[root];
        for (long child = 2 * root + 1; child < end; child = 2 * root + 1) {   // sift row[start] down
            if (child + 1 < end && row[child + 1] > row[child]) ++child;
            if (!(row[child] > x)) break;
            row[root] = row[child];
            root = child;
        }
        row[root] = x;
    }
}

// ---- serial host forms: the definition the kernels are held to (never compiled into a kernel) -------------------------------------

#if !defined(__HIP_DEVICE_COMPILE__)

// canon [Nv].  table [slots] is scratch, slots as slots_ok wants them.  Vertices are inserted in ascending order, so the one
// that claims a slot is the smallest of those that coincide.
inline void host_weld(const float* vertices, long Nv, bool weld, int* table, long slots, int* canon) {
    for (long s = 0; s < slots; ++s) table[s] = -1;
    for (long v = 0; v < Nv; ++v) {
        const float* p = vertices + 3 * v;
        canon[v] = (int)v;
        if (!weld || !finite3(p)) continue;
        for (unsigned long long s = position_hash(p) & (unsigned long long)(slots - 1);; s = (s + 1) & (unsigned long long)(slots - 1)) {
            if (table[s] < 0) {
                table[s] = (int)v;
                break;
            }
            if (same_position(vertices + 3l * table[s], p)) {
                canon[v] = table[s];
                break;
            }
        }
    }
}

inline int host_find(int* parent, int x) {
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

// labels [Nv], tri_labels [Nt]; parent [Nv] is scratch.  `vertices` may be NULL (mesh_components: no position is looked at).
inline void host_components(const float* vertices, const int* triangles, long Nv, long Nt, const int* canon, int* parent, int* labels,
                            int* tri_labels) {
    for (long v = 0; v < Nv; ++v) {
        parent[v] = (int)v;
        labels[v] = -1;
    }
    for (long t = 0; t < Nt; ++t) {
        const int a = canon[triangles[3 * t]], b = canon[triangles[3 * t + 1]], c = canon[triangles[3 * t + 2]];
        tri_labels[t] = -1;
        if (triangle_dropped(vertices, a, b, c)) continue;
        tri_labels[t] = a;
        labels[a] = labels[b] = labels[c] = 0;                                  // used
        const int other[2] = {b, c};
        for (int k = 0; k < 2; ++k) {
            const int x = host_find(parent, a), y = host_find(parent, other[k]);
            if (x < y) parent[y] = x;                                           // the larger root under the smaller
            else parent[x] = y;
        }
    }
    for (long v = 0; v < Nv; ++v)
        if (labels[v] == 0) labels[v] = host_find(parent, (int)v);
    for (long t = 0; t < Nt; ++t)
        if (tri_labels[t] >= 0) tri_labels[t] = labels[tri_labels[t]];
}

// roots / comp_vertices / comp_triangles [components] (room for min(Nv, Nt)), tri_component [Nt]; rank [Nv] is scratch
// -> the number of components
inline long host_component_table(const int* labels, const int* tri_labels, long Nv, long Nt, int* rank, int* roots, int* comp_vertices,
                                 int* comp_triangles, int* tri_component) {
    long n = 0;
    for (long v = 0; v < Nv; ++v) {
        rank[v] = -1;
        if (labels[v] != (int)v) continue;
        roots[n] = (int)v;
        comp_vertices[n] = comp_triangles[n] = 0;
        rank[v] = (int)n++;
    }
    for (long v = 0; v < Nv; ++v)
        if (labels[v] >= 0) ++comp_vertices[rank[labels[v]]];
    for (long t = 0; t < Nt; ++t) {
        tri_component[t] = tri_labels[t] >= 0 ? rank[tri_labels[t]] : -1;
        if (tri_labels[t] >= 0) ++comp_triangles[tri_component[t]];
    }
    return n;
}

// comp_keep [components] -> the number kept
inline long host_select(const int* roots, const int* comp_triangles, long components, long min_triangles, bool largest_only,
                        unsigned char* comp_keep) {
    unsigned long long best = 0;
    for (long k = 0; k < components; ++k) {
        const unsigned long long key = size_key(comp_triangles[k], roots[k]);
        if (key > best) best = key;
    }
    long kept = 0;
    for (long k = 0; k < components; ++k) {
        comp_keep[k] = component_kept(comp_triangles[k], roots[k], min_triangles, largest_only, best) ? 1 : 0;
        kept += comp_keep[k];
    }
    return kept;
}

// out_* with room for Nv vertices and Nt triangles; colors / out_colors may be NULL; number [Nv] is scratch.  counts[0] = Nv',
// counts[1] = Nt'.
inline void host_compact(const float* vertices, const unsigned char* colors, const int* triangles, long Nv, long Nt, const int* canon,
                         const int* labels, const int* tri_component, const unsigned char* comp_keep, const int* rank_of_root,
                         int* number, float* out_vertices, unsigned char* out_colors, int* out_triangles, long* vertex_index,
                         long* triangle_index, long* counts) {
    long nv = 0, nt = 0;
    for (long v = 0; v < Nv; ++v) {
        number[v] = -1;
        if (labels[v] < 0 || !comp_keep[rank_of_root[labels[v]]]) continue;
        for (int k = 0; k < 3; ++k) {
            out_vertices[3 * nv + k] = vertices[3 * v + k];
            if (colors) out_colors[3 * nv + k] = colors[3 * v + k];
        }
        vertex_index[nv] = v;
        number[v] = (int)nv++;
    }
    for (long t = 0; t < Nt; ++t) {
        if (tri_component[t] < 0 || !comp_keep[tri_component[t]]) continue;
        for (int k = 0; k < 3; ++k) out_triangles[3 * nt + k] = number[canon[triangles[3 * t + k]]];
        triangle_index[nt++] = t;
    }
    counts[0] = nv;
    counts[1] = nt;
}

// normals [Nv,3], valid [Nv]; sums [Nv,3] is scratch.  Triangles are walked in ascending order, so every vertex's sum is.
inline void host_normals(const float* vertices, const int* triangles, long Nv, long Nt, double* sums, float* normals,
                         unsigned char* valid) {
    for (long k = 0; k < 3 * Nv; ++k) sums[k] = 0.0;
    for (long t = 0; t < Nt; ++t) {
        const int* c = triangles + 3 * t;
        double n[3];
        triangle_normal(vertices + 3l * c[0], vertices + 3l * c[1], vertices + 3l * c[2], n);
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) sums[3l * c[k] + a] = sums[3l * c[k] + a] + n[a];
    }
    for (long v = 0; v < Nv; ++v) valid[v] = unit_normal(sums + 3 * v, normals + 3 * v) ? 1 : 0;
}

#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace mesh
