// Host program for tests/test_labels_host.py: csrc/mvs_labels_plan.h compiled with the host compiler.  Prints
//   "S <capacity> <slots>"                       the table behind an output capacity (0: out of range)
//   "F <name> <keys> <found> <dropped>"          a table filled one key at a time by the kernel's bounded probe loop
//   "W <items> <waves> <per wave> <covered>"     the contiguous chunk ranges of the row kernels: covered = every item once
// and "done".  Violations of what cannot be printed as a number (a probe sequence that misses a slot, a key that does not come
// back, a drop after fewer or more than `slots` probes) end the program with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mvs_labels_plan.h"

using namespace mvs_labels_plan;

static void require(bool ok, const char* what) {
    if (ok) return;
    std::printf("FAILED %s\n", what);
    std::exit(1);
}

// the insertion of table_add (mvs_labels.hip) without its atomics; returns the number of probes, *dropped when the table was exhausted
static unsigned long long insert(std::vector<unsigned long long>& keys, std::vector<unsigned long long>& counts, unsigned long long key,
                                 unsigned long long n, bool* dropped) {
    const unsigned long long slots = keys.size();
    *dropped = false;
    for (unsigned long long i = 0; i < slots; ++i) {
        const unsigned long long s = probe_slot(key, i, slots);
        require(s < slots, "probe inside the table");
        if (keys[s] == kEmpty) keys[s] = key;
        if (keys[s] == key) {
            counts[s] += n;
            return i + 1;
        }
    }
    *dropped = true;
    return slots;
}

static void fill(const char* name, unsigned long long slots, const std::vector<unsigned long long>& input) {
    std::vector<unsigned long long> keys(slots, kEmpty), counts(slots, 0);
    long long dropped = 0;
    for (unsigned long long key : input) {
        bool d;
        const unsigned long long probes = insert(keys, counts, key, 3, &d);
        require(!d || probes == slots, "a drop takes exactly `slots` probes");
        dropped += d;
    }
    for (unsigned long long key : input) {      // every key a second time: it must find its own slot again, never a new one
        bool d;
        insert(keys, counts, key, 4, &d);
    }
    long long found = 0;
    for (unsigned long long s = 0; s < slots; ++s) {
        if (keys[s] == kEmpty) continue;
        require(counts[s] == 7, "a slot holds both additions of its key");
        ++found;
    }
    std::printf("F %s %zu %lld %lld\n", name, input.size(), found, dropped);
}

int main() {
    const long long caps[] = {0, 1, 512, 513, 4096, 65536, 1LL << 27, (1LL << 27) + 1};
    for (long long cap : caps) std::printf("S %lld %lld\n", cap, table_slots(cap));

    // keys: the labels come back, and no key is the free marker
    require(key_la(pair_key(0x7fffffff, 5)) == 0x7fffffff && key_lb(pair_key(0x7fffffff, 5)) == 5, "key round trip");
    require(key_la(pair_key(0, 0x7fffffff)) == 0 && key_lb(pair_key(0, 0x7fffffff)) == 0x7fffffff, "key round trip");
    require(pair_key(0x7fffffff, 0x7fffffff) != kEmpty, "no key is the free marker");

    // the probe sequence of a key visits every slot exactly once
    for (unsigned long long key : {pair_key(0, 1), pair_key(1, 0), pair_key(70000, 3), pair_key(0x7fffffff, 0x7fffffff)}) {
        const unsigned long long slots = 2048;
        std::vector<int> seen(slots, 0);
        for (unsigned long long i = 0; i < slots; ++i) ++seen[probe_slot(key, i, slots)];
        for (int v : seen) require(v == 1, "every slot once");
    }

    std::vector<unsigned long long> seam;      // a 64 x 64 tile of the labels arange + 1 against a copy shifted by one row: 4096 - 64 + marginals
    for (int i = 0; i < 4096; ++i) seam.push_back(pair_key(i + 1, i + 65 <= 4096 ? i + 65 : 0));
    fill("seam", (unsigned long long)table_slots(4096), seam);
    std::vector<unsigned long long> many;
    for (int i = 0; i < 1030; ++i) many.push_back(pair_key(3 * i + 1, 100000 + i));
    fill("full", 1024, std::vector<unsigned long long>(many.begin(), many.begin() + 1024));
    fill("beyond", 1024, many);

    const long long cases[][2] = {{10, 4}, {8192, 8192}, {8193, 8192}, {0, 4}, {1000003, 8192}};
    for (const auto& cs : cases) {
        const long long items = cs[0], waves = cs[1], per = chunks_per_wave(items, waves);
        long long next = 0;
        bool covered = true;
        for (long long w = 0; w < waves; ++w) {
            const long long first = w * per, last = first + per < items ? first + per : items;
            if (first >= last) continue;
            covered = covered && first == next;
            next = last;
        }
        covered = covered && next == items;
        std::printf("W %lld %lld %lld %d\n", items, waves, per, covered ? 1 : 0);
    }
    require(grid_blocks(0, 4) == 1 && grid_blocks(9, 4) == 3 && grid_blocks(1LL << 40, 4) == kMaxBlocks, "grid_blocks");
    require(row_chunks(1) == 1 && row_chunks(64) == 1 && row_chunks(65) == 2, "row_chunks");
    const int64_t shape[3] = {1, 4, 6}, lo0[3] = {0, 0, 0}, whole[3] = {1, 4, 6}, wide[3] = {1, 4, 7}, none[3] = {1, 0, 6}, lo1[3] = {0, 1, 0};
    require(box_in_tile(lo0, whole, shape) && !box_in_tile(lo0, wide, shape) && !box_in_tile(lo0, none, shape) && !box_in_tile(lo1, whole, shape), "box_in_tile");
    std::printf("done\n");
    return 0;
}
