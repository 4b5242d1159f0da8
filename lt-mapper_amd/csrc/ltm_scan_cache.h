// ltm_scan_cache.h -- the finished scan range images a context keeps between votes: entries, least-recently-used eviction under a byte cap, staged insertion
// (host only: nothing of HIP in here, any C++17 compiler takes it; tests/test_scan_cache_cpu.py runs it alone against a fake pool)
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <utility>
#include <vector>

// scan2RangeImg depends only on (scan set, image shape, keyframe range): the remove / revert / remove passes of one
// resolution and the three ND / PD filter passes project the same scans again, so finished scan images are kept.
// bytes: what the entry counts against the cap (image, plus the bound image once it has one; the nb maxima are not counted).  q_thr: the threshold qbound was made for.
struct ScanImgEntry { uint64_t ss; int rows, cols; size_t kb, nb; uint32_t* buf; uint32_t* smax; size_t bytes; uint64_t stamp; float* qbound; float q_thr; };

struct ScanCache {
    std::vector<ScanImgEntry> entries;
    uint64_t stamp = 0;                       // the last stamp handed out: larger = used later
    size_t cap = (size_t)3 << 30;             // bytes
    std::function<void(void*)> free_buf;      // where a buffer goes when its entry leaves (the context's pool.free); never called with null

    explicit ScanCache(std::function<void(void*)> f) : free_buf(std::move(f)) {}
    ScanCache(const ScanCache&) = delete; ScanCache& operator=(const ScanCache&) = delete;

    size_t held() const { size_t h = 0; for (const ScanImgEntry& e : entries) h += e.bytes; return h; }
    // the entry of this key, stamped as just used, or null
    ScanImgEntry* find(uint64_t ss, int rows, int cols, size_t kb, size_t nb)
    {
        for (ScanImgEntry& e : entries)
            if (e.ss == ss && e.rows == rows && e.cols == cols && e.kb == kb && e.nb == nb) { e.stamp = ++stamp; return &e; }
        return nullptr;
    }
    void free_buffers(const ScanImgEntry& e)      // an entry under construction may lack any of them
    {
        for (void* p : {(void*)e.buf, (void*)e.smax, (void*)e.qbound}) if (p) free_buf(p);
    }
    void release(size_t i) { free_buffers(entries[i]); entries.erase(entries.begin() + (std::ptrdiff_t)i); }
    // room for `need` more bytes under the cap: the least recently used entries leave, down to an empty cache (one request larger than the cap is still served)
    void make_room(size_t need)
    {
        for (size_t h = held(); !entries.empty() && h + need > cap;) {
            size_t lru = 0;
            for (size_t i = 1; i < entries.size(); ++i) if (entries[i].stamp < entries[lru].stamp) lru = i;
            h -= entries[lru].bytes;
            release(lru);
        }
    }
    ScanImgEntry& insert(ScanImgEntry e) { e.stamp = ++stamp; entries.push_back(e); return entries.back(); }
    void drop(uint64_t ss)      // every entry of scan set `ss`; 0: all
    {
        for (size_t i = 0; i < entries.size();) {
            if (ss == 0 || entries[i].ss == ss) release(i);
            else ++i;
        }
    }
    // an entry without a bound image gains one (not written yet: for no threshold); its bytes count from here on and leave with the entry
    void bound_image(ScanImgEntry& e, float* q, size_t q_bytes) { e.qbound = q; e.bytes += q_bytes; e.q_thr = -1.0f; }
};

// Entries under construction: their buffers belong to the stage until hand_over() and go back through the cache's free_buf when the stage is left without it
// (an allocation or a launch threw), so the cache never holds an image that was not written.  add() first, then fill in the pointers as they are allocated.
struct ScanCacheStage {
    ScanCache& cache;
    std::vector<ScanImgEntry> pending;
    explicit ScanCacheStage(ScanCache& c, size_t n) : cache(c) { pending.reserve(n); }
    ScanCacheStage(const ScanCacheStage&) = delete; ScanCacheStage& operator=(const ScanCacheStage&) = delete;
    ~ScanCacheStage() { for (const ScanImgEntry& e : pending) cache.free_buffers(e); }
    ScanImgEntry& add(uint64_t ss, int rows, int cols, size_t kb, size_t nb, size_t bytes, float q_thr)
    {
        pending.push_back(ScanImgEntry{ss, rows, cols, kb, nb, nullptr, nullptr, bytes, 0, nullptr, q_thr});
        return pending.back();
    }
    void hand_over()
    {
        cache.entries.reserve(cache.entries.size() + pending.size());      // what could throw comes first
        for (const ScanImgEntry& e : pending) cache.insert(e);
        pending.clear();
    }
};
