// ltm_block_table.h -- the per-workgroup owner table of the batched kernels ("batches"): a launch over many small records (keyframes, indices,
// pairs, pieces) gives record r the workgroups [span.block0, span.block0 + span.n_blocks) and a table names the record of every workgroup, so a workgroup
// never straddles two records and its record is uniform.  The host half builds the table and compiles without a HIP header (tests/test_block_table_cpu.py);
// the device half is how a kernel finds its record.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace ltm {

// the workgroups of one record; every record struct of a batched launch has one as its member `span`
struct BlockSpan { uint32_t block0, n_blocks; };

class BlockTable {
public:
    static constexpr uint64_t kMaxBlocks = 0x7fffffffull;      // a grid must stay below it
    explicit BlockTable(uint64_t limit = kMaxBlocks) : limit_(limit) {}
    // ceil(items / per_block) workgroups for `record`, behind those of the records before it (no item: the empty span at the current size).  false, and the
    // table as it was, when it would REACH the limit
    bool add(uint32_t record, uint64_t items, uint32_t per_block, BlockSpan* out)
    {
        const uint64_t nb = items / per_block + (items % per_block ? 1 : 0);
        if ((uint64_t)owner_.size() + nb >= limit_) return false;
        *out = BlockSpan{(uint32_t)owner_.size(), (uint32_t)nb};
        owner_.insert(owner_.end(), (size_t)nb, record);
        return true;
    }
    uint32_t size() const { return (uint32_t)owner_.size(); }
    const std::vector<uint32_t>& owner() const { return owner_; }      // owner()[b]: the record of workgroup b
private:
    std::vector<uint32_t> owner_;
    uint64_t limit_;
};
} // namespace ltm

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace ltm {
namespace {
// The record of this workgroup, by reference (uniform: its loads are scalar), and the first of the PER_BLOCK items of the record that the workgroup takes;
// index (nullable): the record's number.  Internal linkage, like ltm_search_walk.h.
template <int PER_BLOCK, class Rec>
__device__ __forceinline__ const Rec& block_record(const Rec* __restrict__ recs, const uint32_t* __restrict__ owner, uint32_t& first, uint32_t* index = nullptr)
{
    const uint32_t r = owner[blockIdx.x];
    if (index) *index = r;
    const Rec& R = recs[r];
    first = (blockIdx.x - R.span.block0) * (uint32_t)PER_BLOCK;
    return R;
}

} // namespace
} // namespace ltm
#endif
