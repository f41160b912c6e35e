// Host bookkeeping of the mesh components on Z-slab contexts (tsdf_mesh_slab_components / tsdf_mesh_merge_component_seams / tsdf_mesh_slab_link_components;
// include/rgbd_recon_hip.h has the definition), free of HIP: the merge of the slabs' seam lists -- a pure function of its arguments, no context and no
// device -- and the check a slab makes of the links it is handed before any of them reaches a scatter.  abi.cpp calls both; a stand-alone program
// (tests/cpp/mesh_cc_seams_main.cpp) runs this text under the host sanitizers; rgbd-recon_amd/binding.py: merge_mesh_component_seams is its numpy twin.
//
// The merge.  Every slab has labelled its part alone: a local component's root is its smallest vertex, an own vertex (a part's triangle has an own vertex
// and indices into the slab above are larger than own ones).  A local component that touches a seam is named by a root record; an up record (g, r) of
// slab k says "vertex g of slab k + 1 is in my component r", the down record (g, r') of slab k + 1 "g is in my component r'": r ~ r'.  Two components of
// ONE slab may meet only in another slab (two columns joined in the slab above), so the union-find runs over the root records of ALL slabs at once, the
// smaller root on top: a set's top is the whole component's smallest vertex.  Everything is integer and every list is sorted: the result is a function
// of the lists' contents alone.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/rgbd_recon_hip.h"

namespace rr {

// position of `key` in a list sorted by its first word, or -1
template <typename Record>
inline int64_t seam_find(const Record* list, uint64_t n, uint32_t key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint32_t k = *(const uint32_t*)&list[mid];
    if (k == key) return (int64_t)mid;
    if (k < key) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// 0: the lists are acceptable and *component_base[n_slabs], links[sum of n_roots] (slab after slab, a slab's links in the order of its root records)
// and *n_components are written.  Otherwise nothing is written: 1 a NULL array; 2 slabs that overlap, are out of order or leave the 32-bit indices;
// 3 a list that is not strictly ascending; 4 a root outside its slab (a root record's root or rank, or a seam record whose root has no root record);
// 5 a seam record's vertex on the wrong side of the seam; 6 an up record without its down record in the slab above; 7 a component's totals leave 32 bits
inline int merge_component_seams(const tsdf_mesh_component_seams* slabs, uint32_t n_slabs, uint64_t* component_base, tsdf_mesh_component_link* links,
                                 uint64_t* n_components) {
  if (n_slabs && !slabs) return 1;
  std::vector<uint64_t> first(n_slabs + 1u, 0);                         // a slab's first node: its root records are nodes first[k] .. first[k + 1])
  for (uint32_t k = 0; k < n_slabs; ++k) {
    const tsdf_mesh_component_seams& S = slabs[k];
    if ((S.n_down && !S.down) || (S.n_up && !S.up) || (S.n_roots && !S.roots)) return 1;
    if (S.vertex_base + S.n_vertices > 0x100000000ull || S.n_local > S.n_vertices) return 2;
    if (k && S.vertex_base < slabs[k - 1].vertex_base + slabs[k - 1].n_vertices) return 2;
    first[k + 1] = first[k] + S.n_roots;
  }
  if (first[n_slabs] && (!links || !component_base)) return 1;
  for (uint32_t k = 0; k < n_slabs; ++k) {
    const tsdf_mesh_component_seams& S = slabs[k];
    const uint64_t v0 = S.vertex_base, v1 = S.vertex_base + S.n_vertices;
    for (uint64_t i = 0; i < S.n_roots; ++i) {
      const tsdf_mesh_seam_root& r = S.roots[i];
      if (i && (S.roots[i - 1].root >= r.root || S.roots[i - 1].rank >= r.rank)) return 3;
      if (r.root < v0 || r.root >= v1 || r.rank >= S.n_local) return 4;
    }
    for (uint64_t i = 0; i < S.n_down; ++i) {
      const tsdf_mesh_seam_vertex& d = S.down[i];
      if (i && S.down[i - 1].vertex >= d.vertex) return 3;
      if (d.vertex < v0 || d.vertex >= v1 || d.root > d.vertex) return 5;
      if (seam_find(S.roots, S.n_roots, d.root) < 0) return 4;
    }
    for (uint64_t i = 0; i < S.n_up; ++i) {
      const tsdf_mesh_seam_vertex& u = S.up[i];
      if (i && S.up[i - 1].vertex >= u.vertex) return 3;
      if (u.vertex < v1) return 5;
      if (seam_find(S.roots, S.n_roots, u.root) < 0) return 4;
      if (k + 1 == n_slabs || seam_find(slabs[k + 1].down, slabs[k + 1].n_down, u.vertex) < 0) return 6;
    }
  }
  // the union-find: node ids ascend with the roots (slabs in order, a slab's records ascending), so the smaller id is the smaller root
  std::vector<uint64_t> parent(first[n_slabs]);
  for (uint64_t i = 0; i < parent.size(); ++i) parent[i] = i;
  const auto find = [&](uint64_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
  for (uint32_t k = 0; k + 1 < n_slabs; ++k) {
    const tsdf_mesh_component_seams& S = slabs[k];
    const tsdf_mesh_component_seams& A = slabs[k + 1];
    for (uint64_t i = 0; i < S.n_up; ++i) {
      const uint32_t above_root = A.down[seam_find(A.down, A.n_down, S.up[i].vertex)].root;
      const uint64_t a = find(first[k] + (uint64_t)seam_find(S.roots, S.n_roots, S.up[i].root));
      const uint64_t b = find(first[k + 1] + (uint64_t)seam_find(A.roots, A.n_roots, above_root));
      if (a != b) parent[a < b ? b : a] = a < b ? a : b;
    }
  }
  // the whole component's totals, on its top node
  std::vector<uint64_t> nv(parent.size(), 0), nt(parent.size(), 0);
  for (uint32_t k = 0; k < n_slabs; ++k)
    for (uint64_t i = 0; i < slabs[k].n_roots; ++i) {
      const uint64_t top = find(first[k] + i);
      nv[top] += slabs[k].roots[i].n_vertices; nt[top] += slabs[k].roots[i].n_triangles;
      if (nv[top] > 0xffffffffull || nt[top] > 0xffffffffull) return 7;
    }
  // the numbering: a slab owns its local components but for the removed roots (those under a smaller root); a surviving boundary root's number is its
  // slab's base + its rank - the removed roots of the slab before it.  What tsdf_mesh_slab_link_components scans is the same count.
  std::vector<uint64_t> base(n_slabs + 1u, 0);
  std::vector<uint32_t> number(parent.size(), 0);
  for (uint32_t k = 0; k < n_slabs; ++k) {
    uint64_t removed = 0;
    for (uint64_t i = 0; i < slabs[k].n_roots; ++i) {
      const uint64_t node = first[k] + i;
      if (find(node) != node) ++removed;
      else number[node] = (uint32_t)(base[k] + slabs[k].roots[i].rank - removed);
    }
    base[k + 1] = base[k] + slabs[k].n_local - removed;
  }
  for (uint32_t k = 0; k < n_slabs; ++k) {
    component_base[k] = base[k];
    for (uint64_t i = 0; i < slabs[k].n_roots; ++i) {
      const uint64_t node = first[k] + i, top = find(node);
      uint32_t top_slab = k;                                            // (the top lies in this slab or below it)
      while (first[top_slab] > top) --top_slab;
      links[node] = tsdf_mesh_component_link{slabs[k].roots[i].root, slabs[top_slab].roots[top - first[top_slab]].root, number[top], 0u,
                                             (uint32_t)nv[top], (uint32_t)nt[top], 0u, 0u};
    }
  }
  if (n_components) *n_components = base[n_slabs];
  return 0;
}

// The links a slab is handed (tsdf_mesh_slab_link_components) against the root records it exported.  0: every index a launch will use is one the slab
// made itself; 1: another count; 2: links[i].root is not root record i's; 3: final_root above root; 4: a final_root that is neither the root, nor a
// vertex of a slab below, nor another exported root of this slab
inline int component_links_check(const tsdf_mesh_seam_root* roots, uint64_t n_roots, uint64_t vertex_base, const tsdf_mesh_component_link* links, uint64_t n_links) {
  if (n_links != n_roots) return 1;
  for (uint64_t i = 0; i < n_links; ++i) {
    const tsdf_mesh_component_link& l = links[i];
    if (l.root != roots[i].root) return 2;
    if (l.final_root > l.root) return 3;
    if (l.final_root != l.root && l.final_root >= vertex_base && seam_find(roots, n_roots, l.final_root) < 0) return 4;
  }
  return 0;
}

}  // namespace rr
