// ltm_api_fpfh.cpp -- C ABI: FPFH descriptors over the targets of search indices (include/ltm.h, "fpfh"), the counterpart of pcl::FPFHEstimation with
// setKSearch.  Kernels in ltm_k_fpfh.hip.
#include "ltm_internal.h"
#include "ltm_fpfh_bins.h"      // kFpfhBins, kFpfhSize

struct ltm_fpfh : IndexRecordSet {            // blocks: offsets, descriptors and SPFH words
    int k = 0;
    float* desc = nullptr;                    // n_points x 33, every record in its target's original order
    unsigned long long* spfh = nullptr;       // n_points x kFpfhWords
    using IndexRecordSet::IndexRecordSet;
};

const std::vector<uint64_t>& ltm_detail::fpfh_rows(ltm_ctx* c, ltm_fpfh* h, const float** desc)
{
    const ltm_fpfh* s = c->open.fpfh.get(h);
    *desc = s->desc;
    return s->bounds;
}

extern "C" {

int ltm_fpfh_upload(ltm_ctx* c, size_t n_records, const uint64_t* offsets, const float* desc_host, ltm_fpfh** out)
{
    if (out) *out = nullptr;
    return guarded(c, [&] {
        LTM_REQUIRE(out && offsets, "null argument");
        LTM_REQUIRE(n_records < 0x7fffffffull / 16, "too many records");
        LTM_REQUIRE(offsets[0] == 0, "offsets must start at 0");
        for (size_t r = 0; r < n_records; ++r) LTM_REQUIRE(offsets[r] <= offsets[r + 1], "offsets must not decrease");
        const uint64_t np = offsets[n_records];
        LTM_REQUIRE(!np || desc_host, "null argument");
        if (np >= 0x80000000ull) throw Err{LTM_E_UNSUPPORTED, "a descriptor set must have fewer than 2^31 rows in all"};
        std::unique_ptr<ltm_fpfh> made(new ltm_fpfh(c, n_records));      // k stays 0: the rows are the caller's
        made->bounds.assign(offsets, offsets + n_records + 1);
        for (size_t r = 0; r < n_records; ++r)      // n_finite of an uploaded record: its rows without a NaN component
            for (uint64_t i = offsets[r]; i < offsets[r + 1]; ++i) {
                bool nan = false;
                for (int b = 0; b < kFpfhSize; ++b) nan = nan || std::isnan(desc_host[i * kFpfhSize + b]);
                made->n_finite[r] += nan ? 0u : 1u;
            }
        made->offsets = made->blocks.alloc<uint64_t>(n_records + 1);
        made->desc = made->blocks.alloc<float>(np * kFpfhSize);
        made->spfh = made->blocks.alloc<unsigned long long>(np * kFpfhWords);
        h2d(c, made->offsets, made->bounds.data(), (n_records + 1) * sizeof(uint64_t));
        h2d(c, made->desc, desc_host, np * kFpfhSize * sizeof(float));
        if (np) LTM_HIP(hipMemsetAsync(made->spfh, 0, np * kFpfhWords * sizeof(unsigned long long), c->stream));
        *out = c->open.fpfh.adopt(made);
    });
}

int ltm_search_fpfh(ltm_ctx* c, size_t n_idx, ltm_search* const* idx, int k, ltm_fpfh** out)
{
    if (out) *out = nullptr;
    return guarded(c, [&] {
        LTM_REQUIRE(out, "null argument");
        LTM_REQUIRE(k >= 2 && k <= kFpfhMaxK, "k must be in [2, 64]");
        check_listed_indices(n_idx, idx, 0x7fffffffull / 16);
        // everything is checked before the device is touched: an error leaves every index as it was
        std::vector<const float4*> normals(n_idx);
        for (size_t i = 0; i < n_idx; ++i) {
            int nk = 0;
            normals[i] = search_normals(c, idx[i], &nk);      // refuses a handle that is not an index of this context
            LTM_REQUIRE(nk != 0, "an index has no normals (ltm_search_estimate_normals)");
        }
        std::vector<ltm_search*> seen(idx, idx + n_idx);
        std::sort(seen.begin(), seen.end());
        LTM_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "an index is listed twice");

        std::unique_ptr<ltm_fpfh> made(new ltm_fpfh(c, n_idx));      // an error leaves nothing behind: the handle dies with `made`, its blocks with it
        made->k = k;
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
            made->set_record(r, L);
            total_f += S.t.Mf;
        });
        const size_t nr = n_idx, np = made->n_points();
        made->offsets = made->blocks.alloc<uint64_t>(nr + 1);
        made->desc = made->blocks.alloc<float>(np * kFpfhSize);
        made->spfh = made->blocks.alloc<unsigned long long>(np * kFpfhWords);
        h2d(c, made->offsets, made->bounds.data(), (nr + 1) * sizeof(uint64_t));
        if (np) {
            LTM_HIP(hipMemsetAsync(made->spfh, 0, np * kFpfhWords * sizeof(unsigned long long), c->stream));      // non-finite positions and points without a normal: no counts
            unsigned long long* stats = c->fpfh_stats.get(c);
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
        *out = c->open.fpfh.adopt(made);
    });
}

int ltm_fpfh_info(ltm_ctx* c, ltm_fpfh* h, size_t* n_records, size_t* n_points, int* k)
{
    return guarded(c, [&] {
        const ltm_fpfh* s = c->open.fpfh.get(h);
        if (n_records) *n_records = s->n_records();
        if (n_points) *n_points = s->n_points();
        if (k) *k = s->k;
    });
}

int ltm_fpfh_device(ltm_ctx* c, ltm_fpfh* h, const uint64_t** offsets_dev, const float** desc_dev, const void** spfh_dev)
{
    return guarded(c, [&] {
        const ltm_fpfh* s = c->open.fpfh.get(h);
        if (offsets_dev) *offsets_dev = s->offsets;
        if (desc_dev) *desc_dev = s->desc;
        if (spfh_dev) *spfh_dev = s->spfh;
    });
}

int ltm_fpfh_download(ltm_ctx* c, ltm_fpfh* h, uint32_t* n_target, uint32_t* n_finite, float* desc, uint8_t* spfh_counts)
{
    return guarded(c, [&] {
        const ltm_fpfh* s = c->open.fpfh.get(h);
        const size_t np = s->n_points();
        s->record_sizes(n_target, n_finite);
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
    return guarded(c, [&] { c->open.fpfh.free(h); });
}

int ltm_debug_fpfh_stats(ltm_ctx* c, uint64_t* stats, int reset)
{
    return guarded(c, [&] { c->fpfh_stats.read(c, stats, reset); });
}

} // extern "C"
