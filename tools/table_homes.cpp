// table_homes.cpp - prints what kttab::make_geom and kttab::probe_of (kmertools_amd/csrc/kt_table.hpp, compiled for the host)
// answer for the table geometries of tests/test_table_geometries.py: tests/golden/table_homes.json, which the numpy
// restatement of the table's hash (tests/table_model.py: geometry, home_of) is compared with.  Regenerate with
//   hipcc -O1 -std=c++17 -Ikmertools_amd/csrc -Iinclude tools/table_homes.cpp -o /tmp/table_homes && /tmp/table_homes > tests/golden/table_homes.json
// Per k: key 0, the largest canonical k-mer (T..T [C] A..A) and 256 canonical k-mers drawn by a fixed mixer.
//   /tmp/table_homes big > tests/golden/table_homes_big.json
// prints the same for the five shapes of tests/big_tables.py - tables of 2^32 bytes and more, up to 5 * 2^30 slots - and 16 or
// so keys each: key 0, the largest canonical k-mer, eight of the mixer's and, BUILT with ktd::khash_inv / ktd::nhash_inv, per
// edge inside the table (slot 2^28: byte 2^32; 2^31; 2^32) one canonical k-mer homed just below the edge and one homed at it,
// one homed in the last position of range 0 and one in the table's last slot.
#include "kt_table.hpp"

#include <cstdio>
#include <string>
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

// a canonical k-mer homed at slot `want` of a table of shape g: the hash bits above the table's n are chosen, the bits below
// drawn by the mixer until the word that khash_inv gives back is a canonical k-mer (k <= 16, a table of 4^k slots: the one
// word nhash_inv gives for the slot; when it is not canonical the next slot towards `step` is taken)
static uint64_t key_homed_at(uint64_t want, int step, const kttab::Geom &g, int k) {
    const uint32_t rs = g.range_slots();
    if (g.kbits) {
        for (uint64_t s = want;; s += (uint64_t)(int64_t)step) {
            const uint64_t key = ktd::nhash_inv((uint32_t)s, g.kbits);
            if (key <= ktd::rev_comp(key, k)) return key;
        }
    }
    const uint64_t r = want / rs, pos = want % rs;
    uint64_t low13 = 0;
    while (((low13 * g.m8) >> 3) != pos) low13++;  // (m8 <= 8: every position has hash bits that scale to it)
    const uint64_t top = (r << kttab::LOG2_RANGE | low13) << g.shift;
    uint64_t z = 0x13198A2E03707344ull + want;
    for (;;) {
        z += 0x9E3779B97F4A7C15ull;
        uint64_t x = z;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        x = (x ^ (x >> 31)) & ((1ull << g.shift) - 1);
        const uint64_t key = ktd::khash_inv(top | x);
        if (key >> (2 * k) == 0 && key <= ktd::rev_comp(key, k)) return key;
    }
}

static int big() {
    struct Shape { const char *name; uint64_t request; int k; };
    const Shape shapes[] = {{"A", 1ull << 28, 31}, {"B", 5ull << 26, 31}, {"E", 5ull << 30, 31}, {"D14", 1ull << 28, 14}, {"D16", 1ull << 32, 16}};
    const uint64_t edges[] = {1ull << 28, 1ull << 31, 1ull << 32};
    printf("{\"tables\": [");
    bool first = true;
    for (const Shape &s : shapes) {
        const kttab::Geom g = kttab::make_geom(s.request, s.k);
        std::vector<uint64_t> keys = keys_of(s.k);
        keys.resize(10);
        for (uint64_t e : edges)
            if (e < g.cap) {
                keys.push_back(key_homed_at(e - 1, -1, g, s.k));
                keys.push_back(key_homed_at(e, 1, g, s.k));
            }
        keys.push_back(key_homed_at(g.range_slots() - 1, -1, g, s.k));
        keys.push_back(key_homed_at(g.cap - 1, -1, g, s.k));
        printf("%s\n {\"name\": \"%s\", \"request\": %llu, \"k\": %d, \"cap\": %llu, \"shift\": %u, \"m8\": %u, \"range_slots\": %u, \"kbits\": %u,\n  \"keys\": [",
               first ? "" : ",", s.name, (unsigned long long)s.request, s.k, (unsigned long long)g.cap, g.shift, g.m8, g.range_slots(), g.kbits);
        first = false;
        for (size_t i = 0; i < keys.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)keys[i]);
        printf("],\n  \"base\": [");
        for (size_t i = 0; i < keys.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)kttab::probe_of(keys[i], g).base);
        printf("],\n  \"rel\": [");
        for (size_t i = 0; i < keys.size(); i++) printf("%s%u", i ? ", " : "", kttab::probe_of(keys[i], g).rel);
        printf("]}");
    }
    printf("]}\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "big") return big();
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
