// Host build of mvster_amd/csrc/mesh_math.h -- TEST INFRASTRUCTURE ONLY.
// The serial host forms of the header (weld, components, selection, compaction, vertex normals) behind a C interface, with the
// very functions the kernels of geo_mesh_clean.hip inline.  Never loaded by the product.
// Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/mesh_clean_cases.py).
#include <vector>

#include "../../mvster_amd/csrc/mesh_math.h"

namespace {

long slots_for(long Nv) {
    long s = mesh::kMinSlots;
    while (s < 2 * Nv) s *= 2;
    return s;
}

}  // namespace

extern "C" {

// canon [Nv]
void hm_mesh_weld(const float* vertices, long Nv, int weld, int* canon) {
    std::vector<int> table(slots_for(Nv));
    mesh::host_weld(vertices, Nv, weld != 0, table.data(), (long)table.size(), canon);
}

// vertices may be NULL and canon may be NULL (the identity).  labels [Nv], tri_labels / tri_component [Nt], roots /
// comp_vertices / comp_triangles with room for min(Nv, Nt) rows -> the number of components
long hm_mesh_components(const float* vertices, const int* triangles, long Nv, long Nt, const int* canon, int* labels, int* tri_labels,
                        int* tri_component, int* roots, int* comp_vertices, int* comp_triangles) {
    std::vector<int> id(Nv), parent(Nv), rank(Nv);
    for (long v = 0; v < Nv; ++v) id[v] = (int)v;
    mesh::host_components(vertices, triangles, Nv, Nt, canon ? canon : id.data(), parent.data(), labels, tri_labels);
    return mesh::host_component_table(labels, tri_labels, Nv, Nt, rank.data(), roots, comp_vertices, comp_triangles, tri_component);
}

// The whole of clean_mesh.  colors / out_colors may be NULL.  out_* with room for Nv vertices and Nt triangles.
// stats [6] = Nv', Nt', components, canonical vertices, dropped triangles, components kept.
void hm_mesh_clean(const float* vertices, const unsigned char* colors, const int* triangles, long Nv, long Nt, int weld,
                   long min_triangles, int largest_only, float* out_vertices, unsigned char* out_colors, int* out_triangles,
                   long* vertex_index, long* triangle_index, long* stats) {
    std::vector<int> table(slots_for(Nv)), canon(Nv), parent(Nv), labels(Nv), rank(Nv), number(Nv), tri_labels(Nt), tri_component(Nt);
    const long rows = Nv < Nt ? Nv : Nt;
    std::vector<int> roots(rows), comp_vertices(rows), comp_triangles(rows);
    std::vector<unsigned char> keep(rows);
    mesh::host_weld(vertices, Nv, weld != 0, table.data(), (long)table.size(), canon.data());
    mesh::host_components(vertices, triangles, Nv, Nt, canon.data(), parent.data(), labels.data(), tri_labels.data());
    const long n = mesh::host_component_table(labels.data(), tri_labels.data(), Nv, Nt, rank.data(), roots.data(), comp_vertices.data(),
                                              comp_triangles.data(), tri_component.data());
    const long kept = mesh::host_select(roots.data(), comp_triangles.data(), n, min_triangles, largest_only != 0, keep.data());
    mesh::host_compact(vertices, colors, triangles, Nv, Nt, canon.data(), labels.data(), tri_component.data(), keep.data(), rank.data(),
                       number.data(), out_vertices, out_colors, out_triangles, vertex_index, triangle_index, stats);
    long canonical = 0, dropped = 0;
    for (long v = 0; v < Nv; ++v) canonical += canon[v] == (int)v;
    for (long t = 0; t < Nt; ++t) dropped += tri_labels[t] < 0;
    stats[2] = n;
    stats[3] = canonical;
    stats[4] = dropped;
    stats[5] = kept;
}

// normals [Nv,3] float32, valid [Nv] uint8
void hm_mesh_normals(const float* vertices, const int* triangles, long Nv, long Nt, float* normals, unsigned char* valid) {
    std::vector<double> sums(3 * Nv);
    mesh::host_normals(vertices, triangles, Nv, Nt, sums.data(), normals, valid);
}

// a row of triangle numbers into ascending order in place (the kernels' own sort)
void hm_mesh_sort_row(int* row, long L) { mesh::sort_row(row, L); }

}  // extern "C"
