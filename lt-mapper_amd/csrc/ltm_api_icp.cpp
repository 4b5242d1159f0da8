// ltm_api_icp.cpp -- C ABI: batched point-to-point, point-to-plane and generalized ICP of source clouds (generalized: source indices) against search indices, the counterpart of the pcl::IterativeClosestPoint runs
// of LTslam::doICPVirtualRelative / doICPGlobalRelative (ltslam/src/LTslam.cpp:187-301) for all the pairs of addSCloops / addRSloops (:370-416, :508-560)
// at once.  Kernels in ltm_k_icp.hip; the arithmetic is stated in include/ltm.h, "icp", "icp, point-to-plane" and "icp, generalized" (one driver, the method is a switch).
#include "ltm_internal.h"

namespace {

// iterations enqueued between two looks at the "pairs not stopped yet" counter (a host round trip each).  LTM_ICP_POLL overrides it (A/B, tools/bench_icp.py)
int poll_interval()
{
    const char* e = getenv("LTM_ICP_POLL");
    const int v = e ? atoi(e) : 0;
    return v >= 1 ? v : 4;
}

void check_params(const ltm_icp_params& p)
{
    LTM_REQUIRE(!std::isnan(p.max_corr_dist) && p.max_corr_dist >= 0.0, "max_corr_dist must be >= 0");
    LTM_REQUIRE(!std::isnan(p.transformation_epsilon) && !std::isnan(p.euclidean_fitness_epsilon), "an epsilon is NaN");
    LTM_REQUIRE(p.max_iterations <= (1 << 20), "max_iterations must be at most 2^20");
}

// the routine behind all entry points: source_of(i) names the points of pair i's source (a cloud, a keyframe of a scan set read in place, or -- generalized
// ICP -- the points and normals of a search index read in place, in the index's own order).  method: kIcpPoint, kIcpPlane or kIcpGicp
struct IcpSource { const float4* d; size_t n; const float4* nrm; };
template <class SourceOf>
void icp_align_impl(ltm_ctx* c, int method, size_t n_pairs, ltm_search* const* targets, SourceOf&& source_of, const double* init16, const ltm_icp_params* params,
                    ltm_icp_result* results, double* trace, double gicp_epsilon = 0.0)
{
    const bool gicp = method == kIcpGicp, plane = method == kIcpPlane;
    const bool wide = gicp || plane;      // records of kIcpPlanePartial doubles, the 6 x 6 solve
    ltm_icp_params prm;
    ltm_icp_default_params(&prm);
    if (params) prm = *params;
    check_params(prm);
    if (!n_pairs) return;
    LTM_REQUIRE(targets && results, "null argument");
    LTM_REQUIRE(n_pairs < 0x7fffffffull, "too many pairs");
    const int max_it = prm.max_iterations;
    const size_t trace_n = trace && max_it > 0 ? n_pairs * (size_t)max_it * 2 : 0;

    // the batch: every pair's slice of the concatenated sources and of the correspondence grid.  A pair with nothing to do (empty source, empty
    // target, no iteration allowed) gets no point and no workgroup and keeps the state it starts with
    std::vector<IcpPair> pairs(n_pairs);
    std::vector<IcpState> st(n_pairs);
    std::vector<uint64_t> off(n_pairs + 1, 0);
    BlockTable table;
    uint32_t active = 0;
    for (size_t i = 0; i < n_pairs; ++i) {
        IcpPair& P = pairs[i];
        memset(&P, 0, sizeof P);
        search_view(c, targets[i], &P.t, &P.f);
        if (wide) {
            int nk = 0;
            P.nrm = search_normals(c, targets[i], &nk);
            LTM_REQUIRE(nk != 0, "a target has no normals (ltm_search_estimate_normals)");
        }
        const IcpSource src = source_of(i);
        LTM_REQUIRE(src.n < 0x80000000ull, "a source must have fewer than 2^31 points");
        const bool run = src.n && P.t.Mf && max_it >= 1;
        P.src = src.d;
        P.snrm = src.nrm;
        P.o[0] = P.f.ox; P.o[1] = P.f.oy; P.o[2] = P.f.oz;
        P.first = off[i];
        P.n = P.n_gather = run ? (uint32_t)src.n : 0u;
        off[i + 1] = off[i] + P.n;
        LTM_REQUIRE(off[i + 1] < 0x80000000ull, "the sources of one batch must have fewer than 2^31 points in all");
        // (unreachable in practice at the table's default limit: with fewer than 2^31 source points in all, checked above, it would take about 2^31 pairs of one point each)
        if (!table.add((uint32_t)i, P.n, kIcpBlock, &P.span)) throw Err{LTM_E_UNSUPPORTED, "too many source points in one batch of ICP pairs"};
        IcpState& S = st[i];
        memset(&S, 0, sizeof S);
        const double* T0 = init16 ? init16 + 16 * i : nullptr;
        for (int k = 0; k < 12; ++k) {
            S.T[k] = T0 ? T0[k] : (k % 5 == 0 ? 1.0 : 0.0);
            LTM_REQUIRE(std::isfinite(S.T[k]), "an initial transform is not finite");
        }
        S.prev_mse = S.last_mse = S.fitness = DBL_MAX;
        S.done = run ? 0 : 1;
        active += run ? 1u : 0u;
    }
    const size_t total = off[n_pairs];
    const uint32_t n_blocks = table.size();

    if (active) {
        DevBuf d_pairs = to_device(c, pairs), d_st = to_device(c, st), d_off = to_device(c, off), d_bp = to_device(c, table.owner());
        std::unique_ptr<DevBuf> d_sorted;      // the sources in their target's code order; generalized ICP reads its source indices in place and has none
        if (!gicp) d_sorted.reset(new DevBuf(c, total * sizeof(float4)));
        DevBuf d_part(c, (size_t)n_blocks * (wide ? kIcpPlanePartial : kIcpPartial) * sizeof(double)), d_unf(c, 4), d_trace(c, std::max<size_t>(trace_n, 1) * 8);
        h2d(c, d_unf.p, &active, 4);
        if (trace_n) LTM_HIP(hipMemsetAsync(d_trace.p, 0xff, trace_n * 8, c->stream));      // all ones: a NaN
        const IcpPair* dp = d_pairs.as<IcpPair>();
        IcpState* ds = d_st.as<IcpState>();
        const uint32_t* bp = d_bp.as<uint32_t>();
        const float4* sorted = d_sorted ? d_sorted->as<float4>() : nullptr;
        if (sorted) {
            // each source once into the code order of its target's frame: the lanes of a wavefront then walk the same part of the tree
            ProfScope ps(c, "icp_prepare", (double)total, 72.0 * (double)total);
            DevBuf keys(c, total * 8), keys_sorted(c, total * 8), idx(c, total * 4), order(c, total * 4);
            const size_t tb = seg_sort_pairs_temp_bytes(total, n_pairs);
            DevBuf temp(c, tb);
            LTM_HIP(icp_order_sources(dp, bp, n_blocks, n_pairs, d_off.as<uint64_t>(), total, keys.as<uint64_t>(), keys_sorted.as<uint64_t>(), idx.as<uint32_t>(),
                                      order.as<uint32_t>(), d_sorted->as<float4>(), temp.p, tb, c->stream));
        }
        const double max2 = prm.max_corr_dist * prm.max_corr_dist;
        const int poll = poll_interval();
        for (int it = 0; it < max_it;) {
            const int chunk = std::min(poll, max_it - it);
            {
                ProfScope ps(c, "icp_iter", (double)total * chunk, 16.0 * (double)total * chunk, -1.0, false);
                if (ps.cls >= 0) c->prof[ps.cls].launches += 2 * (uint64_t)chunk;
                for (int k = 0; k < chunk; ++k) {
                    LTM_HIP(icp_correspond(dp, ds, bp, n_blocks, sorted, max2, method, d_part.as<double>(), c->stream, 1.0 - gicp_epsilon));
                    LTM_HIP(icp_update(dp, ds, n_pairs, d_part.as<double>(), max_it, prm.transformation_epsilon, prm.euclidean_fitness_epsilon,
                                       trace_n ? d_trace.as<double>() : nullptr, d_unf.as<uint32_t>(), c->stream, wide ? 1 : 0));
                }
            }
            it += chunk;
            if (it >= max_it) break;
            uint32_t left = 0;
            d2h(c, &left, d_unf.p, 4);
            if (!left) break;
        }
        {
            ProfScope ps(c, "icp_fitness", (double)total, 16.0 * (double)total, -1.0, false);
            if (ps.cls >= 0) c->prof[ps.cls].launches += 2;
            LTM_HIP(icp_correspond(dp, ds, bp, n_blocks, sorted, 0.0, kIcpScore, d_part.as<double>(), c->stream));
            LTM_HIP(icp_fitness(dp, ds, n_pairs, d_part.as<double>(), c->stream));
        }
        d2h(c, st.data(), d_st.p, n_pairs * sizeof(IcpState));
        if (trace_n) d2h(c, trace, d_trace.p, trace_n * 8);
    } else if (trace_n) {
        for (size_t k = 0; k < trace_n; ++k) trace[k] = std::nan("");
    }
    for (size_t i = 0; i < n_pairs; ++i) {
        const IcpState& S = st[i];
        ltm_icp_result& r = results[i];
        for (int k = 0; k < 12; ++k) r.T[k] = S.T[k];
        r.T[12] = r.T[13] = r.T[14] = 0.0; r.T[15] = 1.0;
        // a pair that never ran has no 1-NN distance at all; one that ran reports the score pass
        r.fitness = pairs[i].n ? S.fitness : DBL_MAX;
        r.last_mse = S.last_mse;
        r.converged = S.converged; r.iterations = S.iterations; r.state = S.state; r.n_corr = S.n_corr;
    }
}

// the two forms of the sources, shared by the point and plane methods
int align_clouds(ltm_ctx* c, int method, size_t n_pairs, ltm_search* const* targets, const ltm_cloud* sources, const double* init16,
                 const ltm_icp_params* params, ltm_icp_result* results, double* trace)
{
    return guarded(c, [&] {
        LTM_REQUIRE(!n_pairs || sources, "null argument");
        icp_align_impl(c, method, n_pairs, targets, [&](size_t i) { const Cloud& src = get_cloud(c, sources[i]); return IcpSource{src.d, src.n, nullptr}; }, init16, params, results, trace);
    });
}
int align_scanset(ltm_ctx* c, int method, size_t n_pairs, ltm_search* const* targets, ltm_scanset sources, const uint32_t* source_kf, const double* init16,
                  const ltm_icp_params* params, ltm_icp_result* results, double* trace)
{
    return guarded(c, [&] {
        const ScanSet& ss = get_ss(c, sources);
        LTM_REQUIRE(!n_pairs || source_kf, "null argument");
        icp_align_impl(c, method, n_pairs, targets, [&](size_t i) {
            LTM_REQUIRE(source_kf[i] < ss.nkf(), "source keyframe out of range");
            return IcpSource{ss.d + ss.off[source_kf[i]], (size_t)(ss.off[source_kf[i] + 1] - ss.off[source_kf[i]]), nullptr};
        }, init16, params, results, trace);
    });
}

} // namespace

extern "C" {

void ltm_icp_default_params(ltm_icp_params* p)
{
    if (!p) return;
    p->max_corr_dist = 150.0;
    p->max_iterations = 100;
    p->transformation_epsilon = 1e-6;
    p->euclidean_fitness_epsilon = 1e-6;
}

int ltm_icp_align(ltm_ctx* c, size_t n_pairs, ltm_search* const* targets, const ltm_cloud* sources, const double* init16, const ltm_icp_params* params,
                  ltm_icp_result* results, double* trace)
{
    return align_clouds(c, kIcpPoint, n_pairs, targets, sources, init16, params, results, trace);
}

int ltm_icp_align_scanset(ltm_ctx* c, size_t n_pairs, ltm_search* const* targets, ltm_scanset sources, const uint32_t* source_kf, const double* init16,
                          const ltm_icp_params* params, ltm_icp_result* results, double* trace)
{
    return align_scanset(c, kIcpPoint, n_pairs, targets, sources, source_kf, init16, params, results, trace);
}

int ltm_icp_align_plane(ltm_ctx* c, size_t n_pairs, ltm_search* const* targets, const ltm_cloud* sources, const double* init16, const ltm_icp_params* params,
                        ltm_icp_result* results, double* trace)
{
    return align_clouds(c, kIcpPlane, n_pairs, targets, sources, init16, params, results, trace);
}

int ltm_icp_align_plane_scanset(ltm_ctx* c, size_t n_pairs, ltm_search* const* targets, ltm_scanset sources, const uint32_t* source_kf, const double* init16,
                                const ltm_icp_params* params, ltm_icp_result* results, double* trace)
{
    return align_scanset(c, kIcpPlane, n_pairs, targets, sources, source_kf, init16, params, results, trace);
}

int ltm_icp_align_gicp(ltm_ctx* c, size_t n_pairs, ltm_search* const* targets, ltm_search* const* sources, const double* init16, const ltm_icp_params* params,
                       double gicp_epsilon, ltm_icp_result* results, double* trace)
{
    return guarded(c, [&] {
        LTM_REQUIRE(std::isfinite(gicp_epsilon) && gicp_epsilon > 0.0 && gicp_epsilon <= 1.0, "gicp_epsilon must be in (0, 1]");
        LTM_REQUIRE(!n_pairs || sources, "null argument");
        icp_align_impl(c, kIcpGicp, n_pairs, targets, [&](size_t i) {
            SearchTree st; SearchFrame sf;
            search_view(c, sources[i], &st, &sf);
            int nk = 0;
            const float4* nrm = search_normals(c, sources[i], &nk);
            LTM_REQUIRE(nk != 0, "a source has no normals (ltm_search_estimate_normals)");
            return IcpSource{st.pts, (size_t)st.Mf, nrm};
        }, init16, params, results, trace, gicp_epsilon);
    });
}

} // extern "C"
