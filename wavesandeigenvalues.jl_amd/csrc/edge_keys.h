// Keys of the sorted edge list of a tetrahedral mesh (assemble_p2.hip numbers the P2 edge DoFs with them, bloch.hip finds the twins of
// image edges in the same list): key = min(u, v) * npoints + max(u, v), the list sorted ascending, i.e. by (smaller point, larger point).
#pragma once
#include <hip/hip_runtime.h>

__device__ inline unsigned long long p2_edge_key(int u, int v, unsigned long long np) {
    return (unsigned long long)min(u, v) * np + (unsigned long long)max(u, v);
}

// position of the edge (u, v) in the sorted list, or -1
__device__ inline int p2_find_edge(const unsigned long long *__restrict__ ek, int64_t ne, unsigned long long np, int u, int v) {
    const unsigned long long key = p2_edge_key(u, v, np);
    int64_t lo = 0, hi = ne;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ek[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < ne && ek[lo] == key) ? (int)lo : -1;
}
