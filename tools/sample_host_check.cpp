// sample_host_check.cpp — the host part of the sample-rate stage (statsd-router_amd/csrc/sample_host.hpp) in a
// stand-alone host program, meant for -fsanitize=address,undefined (tests/test_sample_host_check.py): every line is
// a heap block of exactly its size, so a byte read past its end or before its start is reported. Lines with known
// answers, every truncation of them, every single-byte mutation of them and each of them behind 0..32 further name
// bytes (compared with a plain parse written here from the contract with std::string::find), the ladder, the keep
// rule, the rate texts, the rewrite (into a block of exactly the new size), the configurations and the specs.
// Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../statsd-router_amd/csrc/sample_host.hpp"

using namespace srk;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("line %d: %s\n", __LINE__, #c);                 \
            ++fails;                                               \
        }                                                          \
    } while (0)

// the contract, rule by rule
static bool plain(const std::string &line, uint32_t types, uint32_t *ins, uint32_t *bit) {
    if (line.size() < 6 || line.size() > SR_SAMPLE_LINE_MAX || line.back() != '\n') return false;
    const std::string c = line.substr(0, line.size() - 1);
    const size_t p = c.find(':');
    if (p == std::string::npos || p < 1) return false;
    const size_t q = c.find('|', p + 1);
    if (q == std::string::npos || q == p + 1) return false;
    size_t e = c.find('|', q + 1);
    if (e == std::string::npos) e = c.size();
    const std::string t = c.substr(q + 1, e - q - 1);
    const uint32_t b = t == "c" ? SR_VALID_TYPE_C : t == "ms" ? SR_VALID_TYPE_MS : t == "h" ? SR_VALID_TYPE_H
                     : t == "d" ? SR_VALID_TYPE_D : 0u;
    if (!(b & types)) return false;
    if (e != c.size() && !(e + 1 < c.size() && c[e + 1] == '#')) return false;
    *ins = (uint32_t)e;
    *bit = b;
    return true;
}

static long checked = 0, sampleable = 0;

// the header's parse of a heap copy of exactly the line's size, against the plain one
static void both(const std::string &line, uint32_t types) {
    uint8_t *blk = (uint8_t *)malloc(line.size() ? line.size() : 1);
    memcpy(blk, line.data(), line.size());
    uint32_t ins = 0, bit = 0, pins = 0, pbit = 0;
    const int got = sample_parse(blk, line.size(), types, &ins, &bit);
    const bool want = plain(line, types, &pins, &pbit);
    if (got != (want ? 1 : 0) || (want && (ins != pins || bit != pbit))) {
        printf("parse differs (%d vs %d, ins %u vs %u) on a line of %zu bytes: %.40s\n", got, (int)want, ins, pins, line.size(),
               line.c_str());
        ++fails;
    }
    if (want) {   // and the rewrite of it, into exactly its new size
        ++sampleable;
        for (uint32_t j = 1; j < SR_SAMPLE_STEPS; j += 5) {
            const std::string r = sample_rate_text(j);
            const std::string exp = line.substr(0, pins) + "|@" + r + line.substr(pins);
            uint8_t *dst = (uint8_t *)malloc(exp.size());
            const size_t n = sample_rewrite(dst, blk, line.size(), ins, j);
            if (n != exp.size() || memcmp(dst, exp.data(), n) != 0) {
                printf("rewrite differs at step %u: %.40s\n", j, line.c_str());
                ++fails;
            }
            free(dst);
        }
    }
    free(blk);
    ++checked;
}

int main() {
    const std::vector<std::string> seeds = {
        "svc.req:1|c\n", "svc.req.time:12.5|ms\n", "a.b:3.25|h|#env:prod,zone:a\n", "dist.v:7|d|@0.5\n",
        "lat.p:0020.0020|ms|#k:v,a:b|x\n", "gauge.x:+17|g|#t\n",
        "a-long.name_with/bytes~in.it:18446744073709551615|ms|#a,b,c\n", "x:1|ms||#t\n", "a:1|c\n", "a:1|ms|\n", "a:1|\n",
    };
    const uint32_t type_sets[] = {kSampleTypesAll, SR_VALID_TYPE_MS, kSampleDefaultTypes};
    for (const std::string &ln : seeds) {
        for (uint32_t types : type_sets) {
            for (size_t k = 1; k <= ln.size(); ++k) both(ln.substr(0, k), types);
            for (size_t pad = 0; pad <= 32; ++pad) {
                both(std::string(pad, 'n') + ln, types);
                both(std::string(pad, 'n') + ln.substr(0, ln.size() - 1) + "|#t\n", types);
                both(std::string(pad, 'n') + ln.substr(0, ln.size() - 1) + "|\n", types);
            }
        }
        for (size_t at = 0; at < ln.size(); ++at)
            for (int v = 0; v < 256; ++v) {
                if ((char)v == ln[at]) continue;
                std::string m = ln;
                m[at] = (char)v;
                both(m, kSampleTypesAll);
            }
    }
    // the limits of the length, and long fields
    both("a:" + std::string(1436, '1') + "|h\n", kSampleTypesAll);        // 1441
    both("a:" + std::string(1437, '1') + "|h\n", kSampleTypesAll);        // 1442
    both(std::string(1435, 'n') + ":1|c\n", kSampleTypesAll);
    both("a:1|ms|#" + std::string(1432, 't') + "\n", kSampleTypesAll);
    both("a:1|" + std::string(1400, 'm') + "\n", kSampleTypesAll);
    both("a:" + std::string(1400, '|') + "\n", kSampleTypesAll);
    both(std::string(1000, 'n') + "|" + std::string(400, 'n') + ":1|d\n", kSampleTypesAll);
    both("", kSampleTypesAll);
    CHECK(checked > 30000 && sampleable > 3000);
    {   // the longest rewrite is 1449 bytes
        const std::string ln = "a:" + std::string(1436, '1') + "|h\n";
        std::vector<uint8_t> dst(1449);
        CHECK(sample_rewrite(dst.data(), (const uint8_t *)ln.data(), ln.size(), 1440, 12) == 1449);
        CHECK(memcmp(dst.data() + 1440, "|@0.0001\n", 9) == 0);
        CHECK(sample_rewrite(dst.data(), (const uint8_t *)ln.data(), ln.size(), 1440, 0) == 0);
        CHECK(sample_rewrite(dst.data(), (const uint8_t *)ln.data(), ln.size(), 1440, 13) == 0);
        CHECK(sample_rewrite(dst.data(), (const uint8_t *)ln.data(), ln.size(), 1442, 1) == 0);
    }
    // the ladder, the rate texts and the insert
    static const uint32_t K[SR_SAMPLE_STEPS] = {1, 2, 5, 10, 20, 50, 100, 200, 500, 1000, 2000, 5000, 10000};
    static const char *const R[SR_SAMPLE_STEPS] = {"", "0.5", "0.2", "0.1", "0.05", "0.02", "0.01", "0.005", "0.002", "0.001",
                                                   "0.0005", "0.0002", "0.0001"};
    for (uint32_t j = 0; j < SR_SAMPLE_STEPS; ++j) {
        CHECK(sample_k(j) == K[j]);
        CHECK(strcmp(sample_rate_text(j), R[j]) == 0);
        if (j) {
            uint32_t n = 0;
            const uint64_t text = sample_insert(j, &n);
            const std::string want = std::string("|@") + R[j];
            CHECK(n == want.size() && n == sample_insert_len(j) && n <= SR_SAMPLE_EXTRA_MAX);
            for (uint32_t k = 0; k < 8; ++k) CHECK((uint8_t)(text >> (8 * k)) == (k < n ? (uint8_t)want[k] : 0));
        }
        for (uint32_t limit : {1u, 3u, 0xFFFFFFFFu}) {
            const uint64_t at = (uint64_t)limit * K[j];
            CHECK(sample_step(limit, at) == j);
            CHECK(sample_step(limit, at + 1) == (j + 1 < SR_SAMPLE_STEPS ? j + 1 : j));
        }
    }
    CHECK(sample_rate_text(SR_SAMPLE_STEPS) == nullptr && sample_insert_len(0) == 0);
    CHECK(sample_step(1, 0) == 0 && sample_step(1, ~0ull) == 12 && sample_step(0xFFFFFFFFu, ~0ull) == 12);
    // the keep rule: step 0 keeps everything; at K the kept share of 200,000 draws is about 1 / K; wrapping seeds
    for (uint64_t i = 0; i < 1000; ++i) CHECK(sample_keep(i * 77, ~0ull, i, 0) == 1);
    for (uint32_t j : {1u, 3u, 6u}) {
        long kept = 0;
        for (uint64_t i = 0; i < 200000; ++i) kept += sample_keep(0x1234567ull, ~0ull - 5, i, j);
        const double want = 200000.0 / K[j];
        CHECK(kept > want * 0.9 && kept < want * 1.1);
    }
    CHECK(sample_keep(5, 7, 9, 1) == sample_keep(5, 7, 9, 1));
    // configurations
    sr_sample_config c = {0u, 1u, SR_VALID_TYPE_MS, 0u, 0ull};
    CHECK(sample_check(&c) == 0 && sample_check(nullptr) == -EINVAL);
    for (uint32_t s : {16u, 64u, 65536u, 1u << 22}) { c.slots = s; CHECK(sample_check(&c) == 0); }
    for (uint32_t s : {1u, 8u, 15u, 17u, 48u, 1u << 23, 0x80000000u}) { c.slots = s; CHECK(sample_check(&c) == -EINVAL); }
    c.slots = 0; c.limit = 0; CHECK(sample_check(&c) == -EINVAL);
    c.limit = 1; c.types = 0; CHECK(sample_check(&c) == -EINVAL);
    c.types = SR_VALID_TYPE_G; CHECK(sample_check(&c) == -EINVAL);
    c.types = kSampleTypesAll; c.reserved = 1; CHECK(sample_check(&c) == -EINVAL);
    // specs: each in a heap block of exactly its size and its NUL
    struct Spec { const char *text; int rc; uint32_t limit, types; };
    const Spec specs[] = {
        {"4", 0, 4, kSampleDefaultTypes}, {"4294967295", 0, 0xFFFFFFFFu, kSampleDefaultTypes}, {"1000:c", 0, 1000, SR_VALID_TYPE_C},
        {"7:ms,h,d,c", 0, 7, kSampleTypesAll}, {"5:d,d", 0, 5, SR_VALID_TYPE_D}, {"", -EINVAL, 0, 0}, {"0", -EINVAL, 0, 0},
        {"-1", -EINVAL, 0, 0}, {"+4", -EINVAL, 0, 0}, {"4:", -EINVAL, 0, 0}, {"4:x", -EINVAL, 0, 0}, {"4:c,", -EINVAL, 0, 0},
        {"4:,c", -EINVAL, 0, 0}, {"4:C", -EINVAL, 0, 0}, {"4 ", -EINVAL, 0, 0}, {" 4", -EINVAL, 0, 0}, {"4294967296", -EINVAL, 0, 0},
        {"4:g", -EINVAL, 0, 0}, {"4:m", -EINVAL, 0, 0}, {"4:msx", -EINVAL, 0, 0}, {"99999999999999999999999", -EINVAL, 0, 0},
    };
    for (const Spec &s : specs) {
        const size_t n = strlen(s.text) + 1;
        char *blk = (char *)malloc(n);
        memcpy(blk, s.text, n);
        sr_sample_config out = {9u, 9u, 9u, 9u, 9ull};
        const int rc = sample_parse_spec(blk, &out);
        CHECK(rc == s.rc);
        if (rc == 0) CHECK(out.limit == s.limit && out.types == s.types && out.slots == 0 && out.seed == 0 && out.reserved == 0);
        else CHECK(out.limit == 9u);
        free(blk);
    }
    CHECK(sample_parse_spec(nullptr, &c) == -EINVAL && sample_parse_spec("4", nullptr) == -EINVAL);
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
