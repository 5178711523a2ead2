// table_homes.cpp - prints what kttab::make_geom and kttab::probe_of (kmertools_amd/csrc/kt_table.hpp, compiled for the host)
// answer for the table geometries of tests/test_table_geometries.py: tests/golden/table_homes.json, which the numpy
// restatement of the table's hash (tests/table_model.py: geometry, home_of) is compared with.  Regenerate with
//   hipcc -O1 -std=c++17 -Ikmertools_amd/csrc -Iinclude tools/table_homes.cpp -o /tmp/table_homes && /tmp/table_homes > tests/golden/table_homes.json
// Per k: key 0, the largest canonical k-mer (T..T [C] A..A) and 256 canonical k-mers drawn by a fixed mixer.
#include "kt_table.hpp"

#include <cstdio>
#include <vector>

static std::vector<uint64_t> keys_of(int k) {
    const uint64_t mask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1;
    uint64_t top = 0;  // k / 2 T, a C in the middle of an odd k, k / 2 A
    for (int i = 0; i < k; i++) top = top << 2 | (i < k / 2 ? 3u : (k & 1) && i == k / 2 ? 1u : 0u);
    std::vector<uint64_t> keys{0, top};
    uint64_t z = 0x243F6A8885A308D3ull + (uint64_t)k;
    for (int i = 0; i < 256; i++) {
        z += 0x9E3779B97F4A7C15ull;  // splitmix64
        uint64_t x = z;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        x = (x ^ (x >> 31)) & mask;
        const uint64_t r = ktd::rev_comp(x, k);
        keys.push_back(x < r ? x : r);
    }
    return keys;
}

int main() {
    const uint64_t requests[] = {1024, 4096, 8192, 16384, 20000, 24000, 28000, 32768, 40000, 81920};
    const int ks[] = {7, 8, 15, 16, 17, 21, 31};
    printf("{\"keys\": {");
    for (size_t j = 0; j < sizeof(ks) / sizeof(*ks); j++) {
        const std::vector<uint64_t> keys = keys_of(ks[j]);
        printf("%s\n \"%d\": [", j ? "," : "", ks[j]);
        for (size_t i = 0; i < keys.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)keys[i]);
        printf("]");
    }
    printf("},\n\"tables\": [");
    bool first = true;
    for (uint64_t req : requests)
        for (int k : ks) {
            const kttab::Geom g = kttab::make_geom(req, k);
            const std::vector<uint64_t> keys = keys_of(k);
            printf("%s\n {\"request\": %llu, \"k\": %d, \"cap\": %llu, \"shift\": %u, \"m8\": %u, \"range_slots\": %u, \"kbits\": %u,\n  \"base\": [",
                   first ? "" : ",", (unsigned long long)req, k, (unsigned long long)g.cap, g.shift, g.m8, g.range_slots(), g.kbits);
            first = false;
            for (size_t i = 0; i < keys.size(); i++)
                printf("%s%llu", i ? ", " : "", (unsigned long long)kttab::probe_of(keys[i], g).base);
            printf("],\n  \"rel\": [");
            for (size_t i = 0; i < keys.size(); i++) printf("%s%u", i ? ", " : "", kttab::probe_of(keys[i], g).rel);
            printf("]}");
        }
    printf("]}\n");
    return 0;
}
