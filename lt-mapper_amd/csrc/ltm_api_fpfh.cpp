// ltm_api_fpfh.cpp -- C ABI: FPFH descriptors over the targets of search indices (include/ltm.h, "fpfh"), the counterpart of pcl::FPFHEstimation with
// setKSearch.  Kernels in ltm_k_fpfh.hip.
#include "ltm_internal.h"
#include "ltm_fpfh_bins.h"      // kFpfhBins, kFpfhSize

struct ltm_fpfh {
    ltm_ctx* owner = nullptr;
    PoolBlocks blocks;                        // offsets, descriptors and SPFH words: back in the pool with the handle
    int k = 0;
    std::vector<uint64_t> bounds;             // n_records + 1 positions of the records' targets, from 0
    std::vector<uint32_t> n_finite;           // per record
    uint64_t* offsets = nullptr;              // n_records + 1, the device copy of bounds
    float* desc = nullptr;                    // n_points x 33, every record in its target's original order
    unsigned long long* spfh = nullptr;       // n_points x kFpfhWords
    explicit ltm_fpfh(ltm_ctx* c) : owner(c), blocks(c) {}
    size_t n_records() const { return bounds.size() - 1; }
    size_t n_points() const { return bounds.back(); }
};

namespace {

ltm_fpfh* get_fpfh(ltm_ctx* c, ltm_fpfh* s) { return open_handle(c->fpfh_open, s, "not a descriptor set of this context"); }

// the device counters of ltm_debug_fpfh_stats: outside the pool (they live as long as the context), made on first use
unsigned long long* fpfh_stats_dev(ltm_ctx* c)
{
    if (!c->fpfh_stats_dev) {
        LTM_HIP(hipMalloc(reinterpret_cast<void**>(&c->fpfh_stats_dev), 4 * sizeof(unsigned long long)));
        LTM_HIP(hipMemsetAsync(c->fpfh_stats_dev, 0, 4 * sizeof(unsigned long long), c->stream));
    }
    return c->fpfh_stats_dev;
}

} // namespace

void ltm_detail::fpfh_release_all(ltm_ctx* c)      // ltm_destroy: descriptor sets nobody freed, and the counters
{
    for (ltm_fpfh* s : c->fpfh_open) delete s;
    c->fpfh_open.clear();
    if (c->fpfh_stats_dev) (void)hipFree(c->fpfh_stats_dev);
    c->fpfh_stats_dev = nullptr;
}

extern "C" {

int ltm_search_fpfh(ltm_ctx* c, size_t n_idx, ltm_search* const* idx, int k, ltm_fpfh** out)
{
    if (out) *out = nullptr;
    return guarded(c, [&] {
        LTM_REQUIRE(out, "null argument");
        LTM_REQUIRE(k >= 2 && k <= kFpfhMaxK, "k must be in [2, 64]");
        LTM_REQUIRE(n_idx < 0x7fffffffull / 16, "too many indices");
        LTM_REQUIRE(!n_idx || idx, "null argument");
        // everything is checked before the device is touched: an error leaves every index as it was
        std::vector<const float4*> normals(n_idx);
        for (size_t i = 0; i < n_idx; ++i) {
            LTM_REQUIRE(idx[i], "null search index");
            int nk = 0;
            normals[i] = search_normals(c, idx[i], &nk);      // refuses a handle that is not an index of this context
            LTM_REQUIRE(nk != 0, "an index has no normals (ltm_search_estimate_normals)");
        }
        std::vector<ltm_search*> seen(idx, idx + n_idx);
        std::sort(seen.begin(), seen.end());
        LTM_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "an index is listed twice");

        std::unique_ptr<ltm_fpfh> made(new ltm_fpfh(c));      // an error leaves nothing behind: the handle dies with `made`, its blocks with it
        made->k = k;
        made->bounds.assign(n_idx + 1, 0);
        made->n_finite.assign(n_idx, 0);
        std::vector<FpfhSeg> segs(n_idx);
        BlockTable points;
        uint64_t total_f = 0;
        const char* over_table = "too many target points in one FPFH call";
        for_listed_indices(c, n_idx, idx, points, (uint32_t)fpfh_block(k), true, "the indices of one FPFH call must have fewer than 2^31 target points in all", over_table,
                           [&](size_t r, const ListedIndex& L) {
            FpfhSeg& S = segs[r];
            memset(&S, 0, sizeof S);
            S.t = L.t; S.nrm = normals[r]; S.n_target = L.n_target; S.tbase = L.tbase; S.fbase = L.fbase; S.span = L.span;
            LTM_REQUIRE(!S.t.Mf || S.nrm, "an index has no normals (ltm_search_estimate_normals)");
            made->bounds[r + 1] = L.tbase + L.n_target;
            made->n_finite[r] = S.t.Mf;
            total_f += S.t.Mf;
        });
        const size_t nr = n_idx, np = made->n_points();
        made->offsets = made->blocks.alloc<uint64_t>(nr + 1);
        made->desc = made->blocks.alloc<float>(np * kFpfhSize);
        made->spfh = made->blocks.alloc<unsigned long long>(np * kFpfhWords);
        h2d(c, made->offsets, made->bounds.data(), (nr + 1) * sizeof(uint64_t));
        if (np) {
            LTM_HIP(hipMemsetAsync(made->spfh, 0, np * kFpfhWords * sizeof(unsigned long long), c->stream));      // non-finite positions and points without a normal: no counts
            unsigned long long* stats = fpfh_stats_dev(c);
            // per finite point and neighbour: 32 B of point and normal in pass 1, 32 B of words in pass 2; 164 B written per position
            ProfScope ps(c, "fpfh", (double)total_f * (double)k, (double)total_f * (double)k * 64.0 + 164.0 * (double)np);
            DevBuf d_segs = to_device(c, segs), d_points = to_device(c, points.owner());      // uploads: nothing is read back
            // the neighbour lists of the SPFH pass kept for the weights where they fit the budget and the pool has the memory; otherwise (and with the
            // context switch LTM_FPFH_LISTS=0) the weights collect the neighbourhoods again: the same lists, the same bytes either way
            std::unique_ptr<DevBuf> lists;
            const uint64_t list_bytes = total_f * (uint64_t)k * 8u;
            if (c->fpfh_lists && total_f && list_bytes <= kFpfhListBudget) {
                try { lists.reset(new DevBuf(c, list_bytes)); } catch (const Err& e) { if (e.code != LTM_E_NOMEM) throw; (void)hipGetLastError(); }
            }
            float* list_d2 = lists ? lists->as<float>() : nullptr;
            int* list_idx = lists ? reinterpret_cast<int*>(lists->as<float>() + total_f * (uint64_t)k) : nullptr;
            LTM_HIP(fpfh_estimate(d_segs.as<FpfhSeg>(), d_points.as<uint32_t>(), points.size(), np, k, made->spfh, made->desc, list_d2, list_idx, total_f, stats,
                                  c->stream));
        }
        c->fpfh_open.push_back(made.get());
        *out = made.release();
    });
}

int ltm_fpfh_info(ltm_ctx* c, ltm_fpfh* h, size_t* n_records, size_t* n_points, int* k)
{
    return guarded(c, [&] {
        const ltm_fpfh* s = get_fpfh(c, h);
        if (n_records) *n_records = s->n_records();
        if (n_points) *n_points = s->n_points();
        if (k) *k = s->k;
    });
}

int ltm_fpfh_device(ltm_ctx* c, ltm_fpfh* h, const uint64_t** offsets_dev, const float** desc_dev, const void** spfh_dev)
{
    return guarded(c, [&] {
        const ltm_fpfh* s = get_fpfh(c, h);
        if (offsets_dev) *offsets_dev = s->offsets;
        if (desc_dev) *desc_dev = s->desc;
        if (spfh_dev) *spfh_dev = s->spfh;
    });
}

int ltm_fpfh_download(ltm_ctx* c, ltm_fpfh* h, uint32_t* n_target, uint32_t* n_finite, float* desc, uint8_t* spfh_counts)
{
    return guarded(c, [&] {
        const ltm_fpfh* s = get_fpfh(c, h);
        const size_t nr = s->n_records(), np = s->n_points();
        for (size_t r = 0; r < nr; ++r) {
            if (n_target) n_target[r] = (uint32_t)(s->bounds[r + 1] - s->bounds[r]);
            if (n_finite) n_finite[r] = s->n_finite[r];
        }
        if (desc && np) d2h(c, desc, s->desc, np * kFpfhSize * sizeof(float));
        if (spfh_counts && np) {
            std::vector<unsigned long long> w(np * kFpfhWords);
            d2h(c, w.data(), s->spfh, w.size() * sizeof(unsigned long long));
            for (size_t i = 0; i < np; ++i) {
                const unsigned long long pairs = w[kFpfhWords * i + 3];
                for (int g = 0; g < 3; ++g) {
                    unsigned long long rest = pairs;
                    for (int b = 0; b < kFpfhBins - 1; ++b) {
                        const unsigned long long cnt = (w[kFpfhWords * i + g] >> (6 * b)) & 63ull;
                        rest -= cnt;
                        spfh_counts[kFpfhSize * i + g * kFpfhBins + b] = (uint8_t)cnt;
                    }
                    spfh_counts[kFpfhSize * i + g * kFpfhBins + kFpfhBins - 1] = (uint8_t)rest;
                }
            }
        }
    });
}

int ltm_fpfh_free(ltm_ctx* c, ltm_fpfh* h)
{
    return guarded(c, [&] {
        get_fpfh(c, h);
        forget_handle(c->fpfh_open, h);
        delete h;
    });
}

int ltm_debug_fpfh_stats(ltm_ctx* c, uint64_t* stats, int reset)
{
    return guarded(c, [&] {
        if (!c->fpfh_stats_dev) {      // nothing was estimated yet
            if (stats) for (int i = 0; i < 4; ++i) stats[i] = 0;
            return;
        }
        unsigned long long v[4];
        if (stats) { d2h(c, v, c->fpfh_stats_dev, sizeof v); for (int i = 0; i < 4; ++i) stats[i] = v[i]; }
        if (reset) LTM_HIP(hipMemsetAsync(c->fpfh_stats_dev, 0, sizeof v, c->stream));
    });
}

} // extern "C"
