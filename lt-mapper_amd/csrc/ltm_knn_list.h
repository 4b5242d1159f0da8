// ltm_knn_list.h -- the k-best list of the search index's kNN consumers, in a form that also compiles for the host so that the very same insertions can
// be checked alone (tests/test_knn_list_cpu.py).  knn_collect of ltm_search_walk.h fills it for ICP; the search, normals and statistical-filter kernels
// write the same network out in the kernel, over the words they carry (DESIGN.md 4.4a says why), and name this header as its statement.
//
// KnnListReg<KT> keeps the kk <= KT smallest candidates it was given, ascending, in KT registers, sorted by an insertion network of selects.  A candidate
// is (float distance, target index, sorted position) and the order is pair_less: smaller distance, then smaller index.  For kk < KT the first KT - kk
// slots hold a sentinel of distance -1 that every candidate sorts after, so slot KT - 1 is always the kk-th distance (+inf until kk candidates came).
// init(kk), push(d, index, position), kth(), for_each(f) with f(rank, d, index, position) over the live slots in ascending order, and slots(), a handle
// with the same push and kth that is cheap to copy into the closures of a tree walk.  knn_list_dispatch maps a slot count to the list form that holds it.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LTM_KL_FN __host__ __device__ __forceinline__
#define LTM_KL_UNROLL _Pragma("unroll")
#else
#define LTM_KL_FN inline
#define LTM_KL_UNROLL
#endif

namespace ltm {

// (d, i) goes before (bd, bi): smaller distance, then smaller target index
LTM_KL_FN bool pair_less(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

template <int KT>
struct KnnListReg {
    static_assert(KT >= 1, "KT slots");
    float d[KT];
    int w0[KT];           // target index
    uint32_t w1[KT];      // sorted position
    int kk;

    LTM_KL_FN void init(int kk_)
    {
        kk = kk_;
        LTM_KL_UNROLL
        for (int j = 0; j < KT; ++j) { const bool sent = j < KT - kk; d[j] = sent ? -1.0f : __builtin_inff(); w0[j] = sent ? -1 : INT_MAX; w1[j] = 0u; }
    }
    // The slots by address, to be passed and captured BY VALUE (knn_collect): a closure that holds the addresses of the arrays compiles to the code of
    // kernel-local arrays, one that reaches them through a reference to the list keeps more state live (k = 16: 86 registers against 72, two waves fewer)
    struct Slots {
        float* d; int* w0; uint32_t* w1;
        LTM_KL_FN bool before(float c, int i, int j) const { return pair_less(c, i, d[j], w0[j]); }
        LTM_KL_FN void push(float c, int i, uint32_t pos) const
        {
            if (!before(c, i, KT - 1)) return;
            LTM_KL_UNROLL
            for (int j = KT - 1; j > 0; --j) {
                const bool before_prev = before(c, i, j - 1);
                const bool before_this = before(c, i, j);
                const float nd = before_prev ? d[j - 1] : (before_this ? c : d[j]);
                w0[j] = before_prev ? w0[j - 1] : (before_this ? i : w0[j]);
                w1[j] = before_prev ? w1[j - 1] : (before_this ? pos : w1[j]);
                d[j] = nd;
            }
            if (before(c, i, 0)) { d[0] = c; w0[0] = i; w1[0] = pos; }
        }
        LTM_KL_FN float kth() const { return d[KT - 1]; }
    };
    LTM_KL_FN Slots slots() { return Slots{d, w0, w1}; }
    LTM_KL_FN void push(float c, int i, uint32_t pos) { slots().push(c, i, pos); }
    LTM_KL_FN float kth() const { return d[KT - 1]; }
    template <class F> LTM_KL_FN void for_each(F f) const
    {
        LTM_KL_UNROLL
        for (int j = 0; j < KT; ++j) {
            const int r = j - (KT - kk);      // rank of slot j
            if (r >= 0) f(r, d[j], w0[j], w1[j]);
        }
    }
};

// The two limits of a list: up to kKnnListRegSlots slots it is registers, up to kKnnListSlots the [slot][lane] form in LDS that the kernels write out (what
// bounds k of the search, k of the normals and mean_k + 1).  knn_list_dispatch: f(std::integral_constant<int, KT>) with the smallest register form KT of
// {4, 8, 16} (SMALL: of {1, 2, 4, 8, 16}) that holds `slots`, or with KT = 0 for the LDS form
static constexpr int kKnnListRegSlots = 16, kKnnListSlots = 64;
template <bool SMALL, class F> inline void knn_list_dispatch(int slots, F f)
{
    if constexpr (SMALL) {
        if (slots == 1) return f(std::integral_constant<int, 1>{});
        if (slots == 2) return f(std::integral_constant<int, 2>{});
    }
    if (slots <= 4) f(std::integral_constant<int, 4>{});
    else if (slots <= 8) f(std::integral_constant<int, 8>{});
    else if (slots <= kKnnListRegSlots) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 0>{});
}

} // namespace ltm
