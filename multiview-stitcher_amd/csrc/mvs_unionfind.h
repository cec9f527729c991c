// mvs_unionfind.h -- the lock-free union and find of connected-component labelling (mvs_components.hip), written once for the
// device and for the host: the two atomics sit behind a shim (HIP's on the device, the __atomic builtins of the host compiler
// elsewhere), so tests/native/components_host_test.cpp runs the very same loops on CPU threads under the sanitizers.
//
// parent[] is a forest over the linear indices of the foreground voxels.  THE INVARIANT: parent[i] <= i always, and a parent is
// only ever lowered (the one write is an atomic minimum with a smaller index).  From it:
//   - every chase strictly descends, so it ends without a counter;
//   - a retry of the union goes on from a strictly smaller index;
//   - the smallest index of a component never gets a parent below itself, so it is the component's root whatever the order of
//     execution: the root is the component's first voxel in raster order.
// A load may be stale: it then shows an earlier parent of the node, which is a member of the same component and >= the current one,
// so a chase over stale values still descends inside the component.  What a load can NOT do is decide that a node is a root: that
// decision is the value uf_min returns.  No lane waits for another one: no locks, no spinning.
#pragma once

#if defined(__HIPCC__)
#define MVS_UF_HD __host__ __device__
#else
#define MVS_UF_HD
#endif

namespace mvs_unionfind {

// parent[i] as the memory system holds it now (device: served by L2, never by another CU's stale L1 line)
MVS_UF_HD inline int uf_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

// *p = min(*p, v) as one atomic; returns the value *p had
MVS_UF_HD inline int uf_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(p, v);
#else
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
    return old;
#endif
}

// The node the chase from i ends at: a root as far as loads can tell.  Nothing is written: paths are not compressed while unions
// are in flight (the flatten launch does that afterwards).
MVS_UF_HD inline int uf_find(const int* parent, int i) {
    for (;;) {
        const int p = uf_load(parent + i);
        if (p == i) return i;
        i = p;      // p < i
    }
}

// Join the components of a and b.  With ra < rb the chased ends, rb gets ra by an atomic minimum; rb was a root exactly when the
// atomic returns rb.  Otherwise someone lowered parent[rb] first: rb now points to min(old, ra), both members of the joined
// component, and the union goes on with (ra, old), old < rb, which re-joins whatever the minimum replaced.
// Why no join is lost: count as connected what the forest connects together with the pair every unfinished call still holds.  A
// chase replaces a node of the pair by one of its ancestors; the atomic on a root adds the edge the pair stood for; the atomic on a
// node that was no root replaces its edge to `old` by one to min(old, ra) while the pair becomes (ra, old).  None of the three
// disconnects anything, and a call returns only with its pair in one tree.
MVS_UF_HD inline void uf_unite(int* parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;      // both chases met in one node: one tree, stale loads or not
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = uf_min(parent + b, a);
        if (old == b) return;
        b = old;
    }
}

}  // namespace mvs_unionfind
