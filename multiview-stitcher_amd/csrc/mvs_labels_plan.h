// mvs_labels_plan.h -- host-only pure C++ of the label-stitching entry points (mvs_labels.hip): their limits, the key, hash and size
// of the co-occurrence table, the bounded probe sequence and the launch geometry.  No HIP is needed to read it:
// tests/native/labels_plan_host_test.cpp compiles it with the host compiler under the address and undefined-behaviour sanitizers;
// the kernels use the same functions on the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MVS_LABELS_HD __host__ __device__
#else
#define MVS_LABELS_HD
#endif

namespace mvs_labels_plan {

constexpr int kThreads = 256;         // four waves per workgroup in every kernel of the file
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 2048;      // grid cap of the row kernels (256 CUs x 8 workgroups)
constexpr int kBrickX = 64;           // fuse: voxels along x per brick (16 lanes x 4 voxels), the brick of mvs_label_fuse
constexpr int kVPT = 4;
constexpr long long kMaxCountCapacity = 1LL << 31;      // MVS_LABEL_COUNT_MAX_CAPACITY: labels are int32
constexpr long long kMaxPairCapacity = 1LL << 27;       // MVS_LABEL_PAIR_MAX_CAPACITY: a table of 2^28 slots is 4 GiB
constexpr long long kMinTableSlots = 1024;
constexpr unsigned long long kEmpty = ~0ull;            // no key has it: labels are clamped to 0 .. 2^31 - 1, so bit 63 of a key is 0

// ---- the co-occurrence table ----------------------------------------------------------------------------------------------------------
// key of the pair (la, lb), both >= 0
MVS_LABELS_HD inline unsigned long long pair_key(int la, int lb) { return ((unsigned long long)(unsigned int)la << 32) | (unsigned long long)(unsigned int)lb; }
MVS_LABELS_HD inline int key_la(unsigned long long key) { return (int)(key >> 32); }
MVS_LABELS_HD inline int key_lb(unsigned long long key) { return (int)(key & 0xffffffffull); }

// Slots of the table behind an output capacity: the power of two >= 2 * capacity (load <= 1/2 when the triples fit), at least
// kMinTableSlots.  0: capacity out of range.
inline long long table_slots(long long capacity) {
    if (capacity < 1 || capacity > kMaxPairCapacity) return 0;
    long long slots = kMinTableSlots;
    while (slots < 2 * capacity) slots *= 2;
    return slots;
}

// First slot of a key: the finaliser of splitmix64 (Steele, Lea, Flood 2014; public domain), so that the neighbouring label pairs
// of a seam spread over the whole table.
MVS_LABELS_HD inline unsigned long long hash_key(unsigned long long k) {
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}

// Slot of the i-th probe, 0 <= i < slots: linear from the first one, so the slots probes of a key visit every slot once.
MVS_LABELS_HD inline unsigned long long probe_slot(unsigned long long key, unsigned long long i, unsigned long long slots) {
    return (hash_key(key) + i) & (slots - 1ull);
}

// ---- launch geometry ----------------------------------------------------------------------------------------------------------------
// A row of nx voxels is taken in chunks of 64 consecutive voxels, one wave each.
inline long long row_chunks(long long nx) { return (nx + 63) / 64; }

// Workgroups of a launch over `items` items with `per_block` of them in flight per workgroup: at least 1, at most kMaxBlocks.
inline int grid_blocks(long long items, int per_block) {
    const long long want = (items + per_block - 1) / per_block;
    return (int)(want < 1 ? 1 : (want > kMaxBlocks ? kMaxBlocks : want));
}

// The row kernels give every wave ONE contiguous range of chunks -- wave w takes [w * per, min((w + 1) * per, items)) -- so that a
// run of one label (or one pair of labels) that goes on over many chunks stays in one wave's registers.
MVS_LABELS_HD inline long long chunks_per_wave(long long items, long long waves) { return waves < 1 ? items : (items + waves - 1) / waves; }

// The box (lo, n) of a tile of `shape`: inside it and not empty?
inline bool box_in_tile(const int64_t lo[3], const int64_t n[3], const int64_t shape[3]) {
    for (int k = 0; k < 3; ++k)
        if (lo[k] < 0 || n[k] < 1 || lo[k] > shape[k] - n[k]) return false;
    return true;
}

}  // namespace mvs_labels_plan
