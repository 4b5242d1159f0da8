// ltm_api_search.cpp -- C ABI: device-resident search index with exact k-NN and radius queries, the counterpart of the reference's
// pcl::KdTreeFLANN members (Session.cpp:18-23, :404, :457, :471, :489, :592, :627).  Kernels in ltm_k_search.hip.
#include "ltm_internal.h"

struct ltm_search {
    std::shared_ptr<PoolBlocks> blocks;   // what pts / idx / keys / box point into: the index's own, or shared by the indices of one ltm_search_build_scanset
    std::shared_ptr<PoolBlocks> nblock;   // set: normals points into the block of one ltm_search_estimate_normals (released with the last index, or estimated again)
    float4* normals = nullptr;            // (nx, ny, nz, curvature) of pts[j], Mf of them
    int normals_k = 0;                    // 0: none estimated
    size_t n_target = 0;
    uint32_t Mf = 0, L = 0, P = 0;      // finite points, leaves, leaves rounded up to a power of two
    SearchFrame f{};
    float4* pts = nullptr;              // finite target points in Morton order
    uint32_t* idx = nullptr;            // their positions in the target as given
    uint64_t* keys = nullptr;           // their codes (the kNN seed looks the query's code up)
    float4* box = nullptr;              // 2 x 2P float4: (lo, hi) of nodes 1 .. 2P-1
    SearchTree tree() const { return SearchTree{pts, idx, keys, box, Mf, L, P}; }
};
struct ltm_search_result {
    PoolBlocks blocks;                  // off, idx, d2: back in the pool with the handle
    size_t n_query = 0, total = 0;
    uint64_t* off = nullptr; int32_t* idx = nullptr; float* d2 = nullptr;
    explicit ltm_search_result(ltm_ctx* c) : blocks(c) {}
};

namespace {

SearchFrame frame_of(const float mn[3], const float mx[3]);
void build_index(ltm_ctx* c, ltm_search* s, const Cloud& target)
{
    const size_t n = target.n;
    s->n_target = n;
    LTM_REQUIRE(n < 0x80000000ull, "the target must have fewer than 2^31 points");
    if (!n) return;
    ProfScope p(c, "search_build", (double)n, 48.0 * n);
    float mn[3], mx[3];
    s->Mf = read_box(c, mn, mx, [&](uint32_t* bb) { return search_bbox(target.d, n, bb, c->stream); });
    if (!s->Mf) return;
    s->f = frame_of(mn, mx);
    // codes of every point (non-finite: ~0, sorted behind the finite ones) -> the first Mf entries of the sorted arrays are the index
    DevBuf keys(c, n * 8), idx(c, n * 4);
    s->blocks = std::make_shared<PoolBlocks>(c);
    s->keys = s->blocks->alloc<uint64_t>(n);
    s->idx = s->blocks->alloc<uint32_t>(n);
    LTM_HIP(search_keys(target.d, n, s->f, keys.as<uint64_t>(), idx.as<uint32_t>(), c->stream));
    {
        const size_t tb = sort_temp_bytes(n);
        DevBuf temp(c, tb);
        LTM_HIP(sort_pairs_u64(keys.as<uint64_t>(), s->keys, idx.as<uint32_t>(), s->idx, n, 64, temp.p, tb, c->stream));
    }
    s->pts = s->blocks->alloc<float4>(s->Mf);
    LTM_HIP(gather_points(target.d, s->idx, s->Mf, s->pts, c->stream));
    s->L = (s->Mf + kSearchLeaf - 1) / kSearchLeaf;
    s->P = 1;
    while (s->P < s->L) s->P <<= 1;
    s->box = s->blocks->alloc<float4>((size_t)4 * s->P);
    LTM_HIP(search_tree_boxes(s->pts, s->Mf, s->L, s->P, s->box, c->stream));
}

// the frame of an index from the box of its finite points
SearchFrame frame_of(const float mn[3], const float mx[3])
{
    double ext = 0.0;
    for (int d = 0; d < 3; ++d) ext = std::max(ext, (double)mx[d] - (double)mn[d]);
    return SearchFrame{(double)mn[0], (double)mn[1], (double)mn[2], ext > 0.0 ? 2097151.0 / ext : 0.0};
}

// One index per keyframe [kb, ke) of a scan set: the stages of build_index in segmented form, a fixed number of launches and ONE read-back (the boxes and
// finite counts of all keyframes) for the whole batch.  The indices are views into four blocks the batch shares.
void build_index_batch(ltm_ctx* c, const ScanSet& ss, size_t kb, size_t ke, std::vector<std::unique_ptr<ltm_search>>& out)
{
    const size_t nk = ke - kb;
    const uint64_t first = ss.off[kb], total = ss.off[ke] - first;
    if (total >= 0x80000000ull) throw Err{LTM_E_UNSUPPORTED, "a batch of search indices must have fewer than 2^31 points in all"};
    auto batch = std::make_shared<PoolBlocks>(c);
    out.resize(nk);
    std::vector<SearchSeg> segs(nk);
    std::vector<uint64_t> off(nk + 1, 0);
    BlockTable table;
    for (size_t k = 0; k < nk; ++k) {
        out[k].reset(new ltm_search);
        out[k]->n_target = ss.off[kb + k + 1] - ss.off[kb + k];
        SearchSeg& S = segs[k];
        memset(&S, 0, sizeof S);
        S.src = ss.d + ss.off[kb + k];
        S.first = ss.off[kb + k] - first;
        S.n = (uint32_t)out[k]->n_target;
        // (unreachable in practice at the table's default limit: with fewer than 2^31 points in all, checked above, it would take about 2^31 keyframes of one point each)
        if (!table.add((uint32_t)k, S.n, kSearchSegChunk, &S.span)) throw Err{LTM_E_UNSUPPORTED, "too many points in one batch of search indices"};
        off[k + 1] = S.first + S.n;
    }
    if (!total) return;
    const uint32_t n_blocks = table.size();
    ProfScope p(c, "search_build_batch", (double)total, 48.0 * (double)total);
    DevBuf d_segs = to_device(c, segs), d_bs = to_device(c, table.owner()), d_off = to_device(c, off), bb(c, nk * 8 * sizeof(uint32_t));
    LTM_HIP(search_bbox_seg(d_segs.as<SearchSeg>(), nk, d_bs.as<uint32_t>(), n_blocks, bb.as<uint32_t>(), c->stream));
    std::vector<uint32_t> enc(nk * 8);
    d2h(c, enc.data(), bb.p, enc.size() * 4);      // the one read-back: every size below follows from it
    uint64_t box_total = 0;
    for (size_t k = 0; k < nk; ++k) {
        ltm_search* s = out[k].get();
        SearchSeg& S = segs[k];
        s->Mf = S.n_gather = enc[8 * k + 6];
        if (!s->Mf) continue;
        float mn[3], mx[3];
        decode_box(&enc[8 * k], mn, mx);
        s->f = S.f = frame_of(mn, mx);
        s->L = (s->Mf + kSearchLeaf - 1) / kSearchLeaf;
        s->P = 1;
        while (s->P < s->L) s->P <<= 1;
        S.L = s->L; S.P = s->P;
        S.box0 = box_total;
        box_total += (uint64_t)4 * s->P;
    }
    if (!box_total) return;      // no finite point anywhere: every index is a valid empty one
    h2d(c, d_segs.p, segs.data(), nk * sizeof(SearchSeg));
    DevBuf keys(c, total * 8), idx(c, total * 4);
    uint64_t* keys_sorted = batch->alloc<uint64_t>(total);
    uint32_t* order = batch->alloc<uint32_t>(total);
    float4* pts = batch->alloc<float4>(total);
    float4* box = batch->alloc<float4>(box_total);
    {
        const size_t tb = seg_sort_pairs_temp_bytes(total, nk);
        DevBuf temp(c, tb);
        LTM_HIP(search_order_seg(d_segs.as<SearchSeg>(), d_bs.as<uint32_t>(), n_blocks, nk, d_off.as<uint64_t>(), total, keys.as<uint64_t>(), keys_sorted,
                                 idx.as<uint32_t>(), order, pts, temp.p, tb, c->stream));
    }
    LTM_HIP(search_tree_boxes_seg(d_segs.as<SearchSeg>(), nk, pts, box, c->stream));
    for (size_t k = 0; k < nk; ++k) {
        ltm_search* s = out[k].get();
        if (!s->Mf) continue;
        s->blocks = batch;
        s->pts = pts + segs[k].first; s->idx = order + segs[k].first; s->keys = keys_sorted + segs[k].first; s->box = box + segs[k].box0;
    }
}

// the queries in code order under the index's frame
struct QueryOrder {
    DevBuf keys, keys_sorted, idx, order;
    QueryOrder(ltm_ctx* c, const ltm_search* s, const Cloud& q)
        : keys(c, q.n * 8), keys_sorted(c, q.n * 8), idx(c, q.n * 4), order(c, q.n * 4)
    {
        const size_t tb = sort_temp_bytes(q.n);
        DevBuf temp(c, tb);
        LTM_HIP(search_query_order(q.d, q.n, s->f, keys.as<uint64_t>(), keys_sorted.as<uint64_t>(), idx.as<uint32_t>(), order.as<uint32_t>(), temp.p, tb, c->stream));
    }
};

} // namespace

void ltm_detail::search_view(ltm_ctx* c, ltm_search* s, SearchTree* tree, SearchFrame* frame)
{
    c->open.search.get(s);
    *tree = s->tree();
    *frame = s->f;
}

const float4* ltm_detail::search_normals(ltm_ctx* c, ltm_search* s, int* k)
{
    c->open.search.get(s);
    if (k) *k = s->normals_k;
    return s->normals;
}

extern "C" {

int ltm_search_estimate_normals(ltm_ctx* c, size_t n_idx, ltm_search* const* idx, int k, const float* viewpoints3)
{
    return guarded(c, [&] {
        LTM_REQUIRE(k >= 3 && k <= kNormalsMaxK, "k must be in [3, 64]");
        if (!n_idx) return;
        LTM_REQUIRE(idx, "null argument");
        LTM_REQUIRE(n_idx < 0x7fffffffull, "too many indices");
        // everything is checked before anything changes: an error leaves every index as it was
        std::vector<ltm_search*> seen(idx, idx + n_idx);
        for (size_t i = 0; i < n_idx; ++i) c->open.search.get(idx[i]);
        std::sort(seen.begin(), seen.end());
        LTM_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "an index is listed twice");
        const uint32_t block = (uint32_t)normals_block(k);
        std::vector<NormalsSeg> segs(n_idx);
        BlockTable table;
        uint64_t total = 0;
        for (size_t i = 0; i < n_idx; ++i) {
            NormalsSeg& S = segs[i];
            memset(&S, 0, sizeof S);
            S.t = idx[i]->tree();
            for (int d = 0; d < 3; ++d) {
                S.vp[d] = viewpoints3 ? (double)viewpoints3[3 * i + d] : 0.0;
                LTM_REQUIRE(std::isfinite(S.vp[d]), "a viewpoint is not finite");
            }
            LTM_REQUIRE(table.add((uint32_t)i, S.t.Mf, block, &S.span), "too many target points in one call");
            total += S.t.Mf;
        }
        std::shared_ptr<PoolBlocks> nb;
        if (total) {
            nb = std::make_shared<PoolBlocks>(c);
            float4* normals = nb->alloc<float4>(total);
            uint64_t at = 0;
            for (size_t i = 0; i < n_idx; ++i) { segs[i].out = normals + at; at += segs[i].t.Mf; }
            ProfScope ps(c, "normals", (double)total, (double)total * (32.0 + 16.0 * k));
            DevBuf d_segs = to_device(c, segs), d_bs = to_device(c, table.owner());
            LTM_HIP(estimate_normals(d_segs.as<NormalsSeg>(), d_bs.as<uint32_t>(), table.size(), k, c->stream));
        }
        for (size_t i = 0; i < n_idx; ++i) {
            ltm_search* s = idx[i];
            s->normals = segs[i].t.Mf ? segs[i].out : nullptr;
            s->nblock = segs[i].t.Mf ? nb : nullptr;      // the block of an earlier estimate loses this reference
            s->normals_k = k;
        }
    });
}

int ltm_search_normals_info(ltm_ctx* c, ltm_search* s, int* k, const void** normals_dev)
{
    return guarded(c, [&] {
        c->open.search.get(s);
        if (k) *k = s->normals_k;
        if (normals_dev) *normals_dev = s->normals;
    });
}

int ltm_search_normals_download(ltm_ctx* c, ltm_search* s, float* nxyzc_host)
{
    return guarded(c, [&] {
        c->open.search.get(s);
        LTM_REQUIRE(s->normals_k != 0, "the index has no normals (ltm_search_estimate_normals)");
        if (!s->n_target) return;
        LTM_REQUIRE(nxyzc_host, "null argument");
        const float q = std::nanf("");
        for (size_t i = 0; i < s->n_target * 4; ++i) nxyzc_host[i] = q;      // non-finite target points are not in the index
        if (!s->Mf) return;
        std::vector<float4> n(s->Mf);
        std::vector<uint32_t> at(s->Mf);
        d2h(c, n.data(), s->normals, (size_t)s->Mf * sizeof(float4));
        d2h(c, at.data(), s->idx, (size_t)s->Mf * 4);
        for (uint32_t j = 0; j < s->Mf; ++j) {
            if (at[j] >= s->n_target) throw Err{LTM_E_DEVICE, "a position of the index is outside the target"};
            memcpy(nxyzc_host + 4 * (size_t)at[j], &n[j], sizeof(float4));
        }
    });
}

int ltm_search_build(ltm_ctx* c, ltm_cloud htarget, ltm_search** out)
{
    return guarded(c, [&] {
        LTM_REQUIRE(out, "null argument");
        const Cloud target = get_cloud(c, htarget);
        std::unique_ptr<ltm_search> s(new ltm_search);      // an error leaves nothing behind: the handle dies with `s`, its blocks with it
        build_index(c, s.get(), target);
        *out = c->open.search.adopt(s);
    });
}

int ltm_search_build_scanset(ltm_ctx* c, ltm_scanset hss, size_t kf_begin, size_t kf_end, ltm_search** out)
{
    return guarded(c, [&] {
        const ScanSet& ss = get_ss(c, hss);
        LTM_REQUIRE(kf_begin <= kf_end && kf_end <= ss.nkf(), "keyframe range outside the scan set");
        if (kf_begin == kf_end) return;
        LTM_REQUIRE(out, "null argument");
        std::vector<std::unique_ptr<ltm_search>> made;
        // an error leaves nothing behind: the handles die with `made`, the shared blocks with the last reference to the batch, scratch with its DevBufs
        build_index_batch(c, ss, kf_begin, kf_end, made);
        c->open.search.adopt(made, out);
    });
}

int ltm_search_free(ltm_ctx* c, ltm_search* s)
{
    return guarded(c, [&] { c->open.search.free(s); });
}

int ltm_search_info(ltm_ctx* c, ltm_search* s, size_t* n_target, size_t* n_finite)
{
    return guarded(c, [&] {
        c->open.search.get(s);
        if (n_target) *n_target = s->n_target;
        if (n_finite) *n_finite = s->Mf;
    });
}

int ltm_knn_search(ltm_ctx* c, ltm_search* hs, ltm_cloud hquery, int k, int32_t* idx_dev, float* d2_dev)
{
    return guarded(c, [&] {
        const ltm_search* s = c->open.search.get(hs);
        LTM_REQUIRE(k >= 1 && k <= 64, "k must be in [1, 64]");
        const Cloud q = get_cloud(c, hquery);
        if (!q.n) return;
        LTM_REQUIRE(idx_dev && d2_dev, "null output buffer");
        LTM_REQUIRE(q.n < 0x80000000ull, "too many queries");
        ProfScope ps(c, "knn_search", (double)q.n, (double)q.n * (16.0 + 8.0 * k));
        if (!s->Mf) { LTM_HIP(knn_empty_rows(q.n * (size_t)k, idx_dev, d2_dev, c->stream)); return; }
        QueryOrder qo(c, s, q);
        LTM_HIP(knn_search(q.d, q.n, qo.order.as<uint32_t>(), qo.keys_sorted.as<uint64_t>(), s->tree(), k, idx_dev, d2_dev, c->stream));
    });
}

int ltm_radius_search(ltm_ctx* c, ltm_search* hs, ltm_cloud hquery, float radius, int max_nn, ltm_search_result** out)
{
    return guarded(c, [&] {
        const ltm_search* s = c->open.search.get(hs);
        LTM_REQUIRE(out, "null argument");
        LTM_REQUIRE(!std::isnan(radius), "radius is NaN");
        LTM_REQUIRE(max_nn >= 0, "max_nn must be >= 0 (0: no limit)");
        const Cloud q = get_cloud(c, hquery);
        LTM_REQUIRE(q.n < 0x80000000ull, "too many queries");
        const float r2 = (float)((double)radius * (double)radius);
        std::unique_ptr<ltm_search_result> r(new ltm_search_result(c));
        r->n_query = q.n;
        r->off = r->blocks.alloc<uint64_t>(q.n + 1);
        uint64_t tot[2] = {0, 0};      // all hits, hits kept (max_nn)
        if (q.n && s->Mf) {
            QueryOrder qo(c, s, q);
            DevBuf count(c, q.n * 4), full(c, (q.n + 1) * 8), tb2(c, 16);
            {
                ProfScope ps(c, "radius_count", (double)q.n, (double)q.n * 20.0);
                LTM_HIP(radius_count(q.d, q.n, qo.order.as<uint32_t>(), s->tree(), r2, count.as<uint32_t>(), c->stream));
                const size_t tb = radius_scan_temp_bytes(q.n);
                DevBuf temp(c, tb);
                LTM_HIP(radius_offsets(count.as<uint32_t>(), q.n, 0, full.as<uint64_t>(), temp.p, tb, c->stream));
                LTM_HIP(radius_offsets(count.as<uint32_t>(), q.n, (uint32_t)max_nn, r->off, temp.p, tb, c->stream));
            }
            d2d(c, tb2.as<uint64_t>(), full.as<uint64_t>() + q.n, 8);
            d2d(c, tb2.as<uint64_t>() + 1, r->off + q.n, 8);
            d2h(c, tot, tb2.p, 16);      // the one host round trip: the sizes of the outputs
            LTM_REQUIRE(tot[0] < 0x100000000ull, "more than 2^32 hits in one radius search");
            r->total = tot[1];
            r->idx = r->blocks.alloc<int32_t>(std::max<size_t>(tot[1], 1));
            r->d2 = r->blocks.alloc<float>(std::max<size_t>(tot[1], 1));
            if (tot[0]) {
                ProfScope ps(c, "radius_fill", (double)tot[0], (double)q.n * 20.0 + 16.0 * (double)tot[0] + 8.0 * (double)tot[1]);
                DevBuf pairs(c, tot[0] * 8), sorted(c, tot[0] * 8);
                const size_t tb = radius_sort_temp_bytes(tot[0], q.n);
                DevBuf temp(c, tb);
                LTM_HIP(radius_fill(q.d, q.n, qo.order.as<uint32_t>(), s->tree(), r2, full.as<uint64_t>(), tot[0], r->off, pairs.as<uint64_t>(), sorted.as<uint64_t>(),
                                    r->idx, r->d2, temp.p, tb, c->stream));
            }
        } else {
            LTM_HIP(hipMemsetAsync(r->off, 0, (q.n + 1) * sizeof(uint64_t), c->stream));
            r->idx = r->blocks.alloc<int32_t>(1);
            r->d2 = r->blocks.alloc<float>(1);
        }
        *out = c->open.result.adopt(r);
    });
}

int ltm_search_result_info(ltm_ctx* c, ltm_search_result* hr, size_t* n_query, size_t* total, const uint64_t** offsets_dev, const int32_t** idx_dev,
                           const float** d2_dev)
{
    return guarded(c, [&] {
        const ltm_search_result* r = c->open.result.get(hr);
        if (n_query) *n_query = r->n_query;
        if (total) *total = r->total;
        if (offsets_dev) *offsets_dev = r->off;
        if (idx_dev) *idx_dev = r->idx;
        if (d2_dev) *d2_dev = r->d2;
    });
}

int ltm_search_result_free(ltm_ctx* c, ltm_search_result* r)
{
    return guarded(c, [&] { c->open.result.free(r); });
}

int ltm_debug_pool_live(ltm_ctx* c, uint64_t* live_blocks, uint64_t* live_bytes)
{
    return guarded(c, [&] {
        size_t b = 0;
        for (const auto& kv : c->pool.live) b += kv.second;
        if (live_blocks) *live_blocks = c->pool.live.size();
        if (live_bytes) *live_bytes = b;
    });
}

} // extern "C"
