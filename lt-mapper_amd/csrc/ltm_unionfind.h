// ltm_unionfind.h -- the lock-free union-find of the cluster kernels (ltm_k_cluster.hip), in a form that also compiles for the host so that the very same
// find / unite can be run from CPU threads (tests/test_unionfind_cpu.py).  parent[] holds positions local to one index; parent[x] == x marks a root.
//
// Rules
//  - a root is only ever hooked under a SMALLER position, by a compare-and-swap of parent[root] from `root` to `smaller` (device scope on the GPU: it is
//    performed in memory, beyond the eight L2s of the XCDs, which are not coherent with each other);
//  - so every value ever stored in parent[x] is < x, except the initial x itself, and once parent[x] != x it never is x again;
//  - find() may read stale parents: a stale parent[x] is either x (x was a root when the line was fetched) or an earlier parent of x, and every earlier
//    parent of x is still an ancestor of x, because hooks only ever add edges above roots.  find() never writes;
//  - find_compress() also stores, with plain stores, parent[y] = r for the nodes y it walked over (all of them seen as non-roots, hence non-roots for
//    good) with r the end of its walk: an ancestor of y and < y.  No compare-and-swap on a non-root can succeed, so such a store never undoes a hook;
//  - every hook is validated by its compare-and-swap: it succeeds only if hi is a root in memory at that moment.
// What the plain stores assume of the hardware: a compressing store shares its cache line with other positions' parents, some of which another XCD may
// hook by a compare-and-swap in memory while this XCD's L2 still holds the line with their old value.  The L2 writes a dirty line back under a byte
// mask -- only the bytes that were stored to -- so the stale neighbours in the line never reach memory and cannot overwrite such a hook.  (Every store
// path of a GPU rests on this: two workgroups that write neighbouring words of one line from different XCDs would otherwise lose each other's data.)
// With whole-line write-backs the stores would have to be agent-scope atomic stores instead.
// Termination
//  - find: every step moves to a strictly smaller position (a value that is not smaller ends the walk), so it ends after at most x steps;
//  - unite(a, b): a failed compare-and-swap returns the current parent[hi] < hi, from which the next round starts in place of hi.  The pair (a, b)
//    therefore decreases strictly in a + b with every retry, and a + b >= 0: at most a + b retries whatever the other threads do.  No thread ever
//    waits for another one (no lock, no spin on a value someone else has to write).
// Result: when all unite() calls have returned, two positions are in one tree iff they are connected by united pairs, and every tree's root is the
// smallest position of its component, whatever the schedule (a root is smaller than everything below it).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LTM_UF_FN __device__ __forceinline__
#else
#define LTM_UF_FN inline
#endif

namespace ltm {
namespace uf {

LTM_UF_FN uint32_t load(const uint32_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
LTM_UF_FN void store(uint32_t* p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *p = v;
#else
    __atomic_store_n(p, v, __ATOMIC_RELAXED);
#endif
}
// returns the value parent[at] held: `expect` iff the swap was made
LTM_UF_FN uint32_t cas(uint32_t* p, uint32_t expect, uint32_t desired)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, desired);
#else
    uint32_t e = expect;
    __atomic_compare_exchange_n(p, &e, desired, false, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED);
    return e;
#endif
}

LTM_UF_FN uint32_t find(const uint32_t* parent, uint32_t x)
{
    while (true) {
        const uint32_t p = load(parent + x);
        if (p >= x) return x;      // a root (p == x); p > x never occurs and would end the walk as well
        x = p;
    }
}
LTM_UF_FN uint32_t find_compress(uint32_t* parent, uint32_t x)
{
    const uint32_t r = find(parent, x);
    while (true) {
        const uint32_t p = load(parent + x);
        if (p >= x || p <= r) break;      // x is (seen as) a root, or already points at r or above it
        store(parent + x, r);
        x = p;
    }
    return r;
}
// unites the sets of a and b; returns the root it left them under (as seen by this thread) and adds the failed compare-and-swaps to *retries
LTM_UF_FN uint32_t unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t* retries)
{
    while (true) {
        a = find_compress(parent, a);
        b = find_compress(parent, b);
        if (a == b) return a;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = cas(parent + hi, hi, lo);
        if (old == hi) return lo;
        ++*retries;
        a = old;      // < hi: somebody hooked hi meanwhile
        b = lo;
    }
}

} // namespace uf
} // namespace ltm
