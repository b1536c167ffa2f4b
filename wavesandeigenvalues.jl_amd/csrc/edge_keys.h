// Keys of the sorted edge lists of a tetrahedral mesh.  assemble_p2.hip numbers the P2 edge DoFs with p2_edge_key and bloch.hip finds the
// twins of image edges in the same list: key = min(u, v) * npoints + max(u, v), the list sorted ascending, i.e. by (smaller point, larger
// point).  octosplit.hip numbers its midpoints with octo_edge_key, the other order.
#pragma once
#include <hip/hip_runtime.h>

__device__ inline unsigned long long p2_edge_key(int u, int v, unsigned long long np) {
    return (unsigned long long)min(u, v) * np + (unsigned long long)max(u, v);
}

// The reference's own order of mesh.lines (src/Mesh/sorter.jl:9-31: points sorted descending, compared lexicographically), which numbers the
// midpoints of octosplit.hip: key = max(u, v) * npoints + min(u, v), the list sorted ascending, i.e. by (larger point, smaller point).
__device__ inline unsigned long long octo_edge_key(int u, int v, unsigned long long np) {
    return (unsigned long long)max(u, v) * np + (unsigned long long)min(u, v);
}

// position of the key in a sorted list of unique keys, or -1
__device__ inline int edge_key_position(const unsigned long long *__restrict__ ek, int64_t ne, unsigned long long key) {
    int64_t lo = 0, hi = ne;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ek[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < ne && ek[lo] == key) ? (int)lo : -1;
}

// position of the edge (u, v) in the list sorted by p2_edge_key, or -1
__device__ inline int p2_find_edge(const unsigned long long *__restrict__ ek, int64_t ne, unsigned long long np, int u, int v) {
    return edge_key_position(ek, ne, p2_edge_key(u, v, np));
}
