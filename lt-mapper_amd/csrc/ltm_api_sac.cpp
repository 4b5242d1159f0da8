// ltm_api_sac.cpp -- C ABI: feature-space correspondences between records of descriptor sets (include/ltm.h, "fpfh matches") and the sample-consensus
// initial alignment over them ("initial alignment"): the counterparts of pcl::SampleConsensusPrerejective's feature search and computeTransformation.
// Kernels in ltm_k_sac.hip.
#include "ltm_internal.h"

struct ltm_matches : RecordSet {              // one record per pair, its rows the pair's source rows; blocks: offsets, target rows and distances
    int kc = 0;
    std::vector<uint32_t> n_target;           // per record: the rows of the pair's target record
    uint64_t* offsets = nullptr;              // n_records + 1, the device copy of bounds
    int32_t* idx = nullptr;                   // n_points x kc
    float* dist = nullptr;                    // n_points x kc
    using RecordSet::RecordSet;
};

struct ltm_sac : RecordSet {                  // one record per pair (no points of its own); blocks: hyp_counts, hyp_valid and the records' results
    uint32_t max_iterations = 0;
    uint32_t* counts = nullptr;               // n_records x max_iterations
    uint8_t* valid = nullptr;                 // n_records x max_iterations
    SacOut* out = nullptr;                    // n_records
    using RecordSet::RecordSet;
};

extern "C" {

uint32_t ltm_match_tile_rows(void) { return (uint32_t)kMatchTileRows; }

int ltm_fpfh_match(ltm_ctx* c, size_t n_pairs, ltm_fpfh* target_set, const uint32_t* target_rec, ltm_fpfh* source_set, const uint32_t* source_rec, int kc,
                   ltm_matches** out)
{
    if (out) *out = nullptr;
    return guarded(c, [&] {
        LTM_REQUIRE(out, "null argument");
        LTM_REQUIRE(kc >= 1 && kc <= kMatchMaxK, "kc must be in [1, 16]");
        LTM_REQUIRE(n_pairs < 0x7fffffffull / 16, "too many pairs");
        LTM_REQUIRE(!n_pairs || (target_rec && source_rec), "null argument");
        // everything is checked before the device is touched
        const float *tdesc = nullptr, *sdesc = nullptr;
        const std::vector<uint64_t>& tb = fpfh_rows(c, target_set, &tdesc);      // refuses a handle that is not a descriptor set of this context
        const std::vector<uint64_t>& sb = fpfh_rows(c, source_set, &sdesc);
        for (size_t i = 0; i < n_pairs; ++i)
            LTM_REQUIRE((size_t)target_rec[i] + 1 < tb.size() && (size_t)source_rec[i] + 1 < sb.size(), "a record number is outside its descriptor set");

        std::unique_ptr<ltm_matches> made(new ltm_matches(c));      // an error leaves nothing behind: the handle dies with `made`, its blocks with it
        made->kc = kc;
        made->bounds.assign(n_pairs + 1, 0);
        made->n_target.assign(n_pairs, 0);
        std::vector<MatchPair> pairs(n_pairs);
        BlockTable table;
        double work = 0.0;
        for (size_t i = 0; i < n_pairs; ++i) {
            const uint64_t t0 = tb[target_rec[i]], nt = tb[target_rec[i] + 1] - t0, s0 = sb[source_rec[i]], ns = sb[source_rec[i] + 1] - s0;
            MatchPair& P = pairs[i];
            memset(&P, 0, sizeof P);
            P.src = sdesc + s0 * kMatchRow; P.tgt = tdesc + t0 * kMatchRow; P.obase = made->bounds[i];
            P.n_source = (uint32_t)ns; P.n_target = (uint32_t)nt;      // a descriptor set has fewer than 2^31 rows in all
            made->bounds[i + 1] = made->bounds[i] + ns;
            made->n_target[i] = (uint32_t)nt;
            if (made->bounds[i + 1] >= 0x80000000ull) throw Err{LTM_E_UNSUPPORTED, "the pairs of one ltm_fpfh_match must have fewer than 2^31 source rows in all"};
            if (!table.add((uint32_t)i, ns, kMatchBlock, &P.span)) throw Err{LTM_E_UNSUPPORTED, "too many source rows in one ltm_fpfh_match"};
            work += (double)ns * (double)nt;
        }
        const size_t np = made->n_points();
        made->offsets = made->blocks.alloc<uint64_t>(n_pairs + 1);
        made->idx = made->blocks.alloc<int32_t>(np * (size_t)kc);
        made->dist = made->blocks.alloc<float>(np * (size_t)kc);
        h2d(c, made->offsets, made->bounds.data(), (n_pairs + 1) * sizeof(uint64_t));
        if (table.size()) {
            // per workgroup its source rows once and every target row of its pair once; 8 kc bytes written per source row
            ProfScope ps(c, "fpfh_match", work, (double)np * (132.0 + 8.0 * kc) + work / kMatchBlock * 132.0);
            DevBuf d_pairs = to_device(c, pairs), d_owner = to_device(c, table.owner());      // uploads: nothing is read back
            LTM_HIP(fpfh_match(d_pairs.as<MatchPair>(), d_owner.as<uint32_t>(), table.size(), kc, made->idx, made->dist, c->stream));
        }
        *out = c->open.matches.adopt(made);
    });
}

int ltm_matches_info(ltm_ctx* c, ltm_matches* h, size_t* n_pairs, size_t* n_rows, int* kc)
{
    return guarded(c, [&] {
        const ltm_matches* s = c->open.matches.get(h);
        if (n_pairs) *n_pairs = s->n_records();
        if (n_rows) *n_rows = s->n_points();
        if (kc) *kc = s->kc;
    });
}

int ltm_matches_device(ltm_ctx* c, ltm_matches* h, const uint64_t** offsets_dev, const int32_t** indices_dev, const float** distances_dev)
{
    return guarded(c, [&] {
        const ltm_matches* s = c->open.matches.get(h);
        if (offsets_dev) *offsets_dev = s->offsets;
        if (indices_dev) *indices_dev = s->idx;
        if (distances_dev) *distances_dev = s->dist;
    });
}

int ltm_matches_download(ltm_ctx* c, ltm_matches* h, uint32_t* n_source, uint32_t* n_target, int32_t* indices, float* distances)
{
    return guarded(c, [&] {
        const ltm_matches* s = c->open.matches.get(h);
        const size_t n = s->n_points() * (size_t)s->kc;
        for (size_t k = 0; k < s->n_records(); ++k) {
            if (n_source) n_source[k] = (uint32_t)(s->bounds[k + 1] - s->bounds[k]);
            if (n_target) n_target[k] = s->n_target[k];
        }
        if (indices && n) d2h(c, indices, s->idx, n * sizeof(int32_t));
        if (distances && n) d2h(c, distances, s->dist, n * sizeof(float));
    });
}

int ltm_matches_free(ltm_ctx* c, ltm_matches* h)
{
    return guarded(c, [&] { c->open.matches.free(h); });
}

void ltm_sac_default_params(ltm_sac_params* p)
{
    if (!p) return;
    p->max_iterations = 1000;
    p->seed = 0;
    p->similarity_threshold = 0.9;
    p->inlier_distance = 0.0;      // PCL's default is unusable: must be set
    p->inlier_fraction = 0.25;
    p->eval_stride = 1;
}

uint32_t ltm_sac_block_points(void) { return (uint32_t)kSacBlockPoints; }

int ltm_sac_align(ltm_ctx* c, size_t n_pairs, ltm_search* const* targets, ltm_search* const* sources, ltm_matches* matches, const ltm_sac_params* p,
                  ltm_sac** out)
{
    if (out) *out = nullptr;
    return guarded(c, [&] {
        LTM_REQUIRE(out && p, "null argument");
        LTM_REQUIRE(p->max_iterations >= 1 && p->max_iterations <= (uint32_t)kSacMaxIterations, "need 1 <= max_iterations <= 16384");
        LTM_REQUIRE(p->similarity_threshold >= 0.0 && p->similarity_threshold < 1.0, "similarity_threshold must be in [0, 1)");
        LTM_REQUIRE(std::isfinite(p->inlier_distance) && p->inlier_distance > 0.0, "inlier_distance must be finite and > 0");
        LTM_REQUIRE(p->inlier_fraction >= 0.0 && p->inlier_fraction <= 1.0, "inlier_fraction must be in [0, 1]");
        LTM_REQUIRE(p->eval_stride >= 1, "eval_stride must be >= 1");
        const ltm_matches* M = c->open.matches.get(matches);
        LTM_REQUIRE(n_pairs == M->n_records(), "n_pairs is not the match set's number of pairs");
        check_listed_indices(n_pairs, targets, 0x7fffffffull / 16);
        check_listed_indices(n_pairs, sources, 0x7fffffffull / 16);
        // everything is checked before the device is touched.  An index may serve many pairs: one row table per distinct index
        std::map<ltm_search*, size_t> table_of;
        std::vector<SacRows> rows;
        std::vector<SacPair> pairs(n_pairs);
        BlockTable row_blocks, vote_blocks;
        uint64_t n_row_entries = 0;
        double work = 0.0;
        auto rows_of = [&](ltm_search* idx, SearchTree* t, size_t* nt) {
            SearchFrame f;
            search_view(c, idx, t, &f);      // refuses a handle that is not an index of this context
            if (ltm_search_info(c, idx, nt, nullptr) != LTM_OK) throw Err{LTM_E_INVALID, c->err};
            auto it = table_of.find(idx);
            if (it != table_of.end()) return rows[it->second].base;
            SacRows R;
            memset(&R, 0, sizeof R);
            R.idx = t->idx; R.base = n_row_entries; R.Mf = t->Mf;
            if (!row_blocks.add((uint32_t)rows.size(), R.Mf, kSacBlock, &R.span)) throw Err{LTM_E_UNSUPPORTED, "too many points in one ltm_sac_align"};
            n_row_entries += *nt;
            table_of[idx] = rows.size();
            rows.push_back(R);
            return R.base;
        };
        std::vector<uint64_t> tbase(n_pairs), sbase(n_pairs);
        for (size_t i = 0; i < n_pairs; ++i) {
            SacPair& P = pairs[i];
            memset(&P, 0, sizeof P);
            size_t nt = 0, ns = 0;
            tbase[i] = rows_of(targets[i], &P.tt, &nt);
            sbase[i] = rows_of(sources[i], &P.st, &ns);
            LTM_REQUIRE(nt == M->n_target[i] && ns == M->bounds[i + 1] - M->bounds[i], "an index does not have the rows of its match record");
            P.match = M->idx + M->bounds[i] * (size_t)M->kc;
            P.n_rows = (uint32_t)ns;
            P.n_eval = P.st.Mf / p->eval_stride + (P.st.Mf % p->eval_stride ? 1u : 0u);
            if (!vote_blocks.add((uint32_t)i, P.n_eval, kSacBlockPoints, &P.span)) throw Err{LTM_E_UNSUPPORTED, "too many points in one ltm_sac_align"};
            work += (double)P.n_eval * (double)p->max_iterations;
        }
        if (n_row_entries >= 0x80000000ull) throw Err{LTM_E_UNSUPPORTED, "the indices of one ltm_sac_align must have fewer than 2^31 target points in all"};

        std::unique_ptr<ltm_sac> made(new ltm_sac(c));      // an error leaves nothing behind: the handle dies with `made`, its blocks with it, scratch with its DevBufs
        const size_t H = p->max_iterations;
        made->bounds.assign(n_pairs + 1, 0);
        made->max_iterations = p->max_iterations;
        made->counts = made->blocks.alloc<uint32_t>(n_pairs * H);
        made->valid = made->blocks.alloc<uint8_t>(n_pairs * H);
        made->out = made->blocks.alloc<SacOut>(n_pairs);
        if (n_pairs) {
            SacLaunch L;
            memset(&L, 0, sizeof L);
            L.thr2 = p->similarity_threshold * p->similarity_threshold;
            L.r2 = p->inlier_distance * p->inlier_distance;
            L.inlier_fraction = p->inlier_fraction;
            L.max_iterations = p->max_iterations; L.seed = p->seed; L.stride = p->eval_stride; L.kc = M->kc;
            unsigned long long* stats = c->sac_stats.get(c);
            ProfScope ps(c, "sac_align", work, 16.0 * work / (double)H + 96.0 * (double)(n_pairs * H));
            DevBuf row(c, std::max<uint64_t>(n_row_entries, 1) * sizeof(uint32_t)), hyp(c, n_pairs * H * sizeof(SacHyp));
            for (size_t i = 0; i < n_pairs; ++i) { pairs[i].trow = row.as<uint32_t>() + tbase[i]; pairs[i].srow = row.as<uint32_t>() + sbase[i]; }
            DevBuf d_rows = to_device(c, rows), d_row_owner = to_device(c, row_blocks.owner());      // uploads: nothing is read back
            DevBuf d_pairs = to_device(c, pairs), d_owner = to_device(c, vote_blocks.owner());
            LTM_HIP(hipMemsetAsync(row.p, 0xff, std::max<uint64_t>(n_row_entries, 1) * sizeof(uint32_t), c->stream));      // a position without a finite point
            LTM_HIP(hipMemsetAsync(made->counts, 0, n_pairs * H * sizeof(uint32_t), c->stream));
            LTM_HIP(hipMemsetAsync(made->out, 0, n_pairs * sizeof(SacOut), c->stream));
            LTM_HIP(sac_align(d_rows.as<SacRows>(), d_row_owner.as<uint32_t>(), row_blocks.size(), row.as<uint32_t>(), d_pairs.as<SacPair>(), d_owner.as<uint32_t>(),
                              vote_blocks.size(), (uint32_t)n_pairs, L, hyp.as<SacHyp>(), made->valid, made->counts, made->out, stats, c->stream));
        }
        *out = c->open.sac.adopt(made);
    });
}

int ltm_sac_info(ltm_ctx* c, ltm_sac* h, size_t* n_pairs, uint32_t* max_iterations)
{
    return guarded(c, [&] {
        const ltm_sac* s = c->open.sac.get(h);
        if (n_pairs) *n_pairs = s->n_records();
        if (max_iterations) *max_iterations = s->max_iterations;
    });
}

int ltm_sac_device(ltm_ctx* c, ltm_sac* h, const uint32_t** hyp_counts_dev, const uint8_t** hyp_valid_dev)
{
    return guarded(c, [&] {
        const ltm_sac* s = c->open.sac.get(h);
        if (hyp_counts_dev) *hyp_counts_dev = s->counts;
        if (hyp_valid_dev) *hyp_valid_dev = s->valid;
    });
}

int ltm_sac_download(ltm_ctx* c, ltm_sac* h, uint8_t* found, int32_t* best, uint32_t* consensus, uint32_t* n_valid, uint32_t* n_prerejected, uint32_t* n_eval,
                     double* T16, uint32_t* hyp_counts, uint8_t* hyp_valid)
{
    return guarded(c, [&] {
        const ltm_sac* s = c->open.sac.get(h);
        const size_t nr = s->n_records(), H = s->max_iterations;
        if (nr && (found || best || consensus || n_valid || n_prerejected || n_eval || T16)) {
            std::vector<SacOut> o(nr);
            d2h(c, o.data(), s->out, nr * sizeof(SacOut));
            for (size_t k = 0; k < nr; ++k) {
                if (found) found[k] = o[k].found;
                if (best) best[k] = o[k].best;
                if (consensus) consensus[k] = o[k].consensus;
                if (n_valid) n_valid[k] = o[k].n_valid;
                if (n_prerejected) n_prerejected[k] = o[k].n_prerejected;
                if (n_eval) n_eval[k] = o[k].n_eval;
                if (T16) memcpy(T16 + 16 * k, o[k].T, 16 * sizeof(double));
            }
        }
        if (hyp_counts) d2h(c, hyp_counts, s->counts, nr * H * sizeof(uint32_t));
        if (hyp_valid) d2h(c, hyp_valid, s->valid, nr * H);
    });
}

int ltm_sac_free(ltm_ctx* c, ltm_sac* h)
{
    return guarded(c, [&] { c->open.sac.free(h); });
}

int ltm_debug_sac_stats(ltm_ctx* c, uint64_t* stats, int reset)
{
    return guarded(c, [&] { c->sac_stats.read(c, stats, reset); });
}

} // extern "C"
