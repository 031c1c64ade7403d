// coalesce_host_check.cpp — the host functions of the plain-counter coalescing
// (statsd-router_amd/csrc/coalesce_host.hpp) in a stand-alone host program, meant for
// -fsanitize=address,undefined (tests/test_coalesce_host_check.py): every line is a heap block of exactly its
// length and every destination one of exactly the bytes the function may write, so a byte read or written past
// either is reported. Prints "ok".
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../statsd-router_amd/csrc/coalesce_host.hpp"

using namespace srk;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("line %d: %s\n", __LINE__, #c);                 \
            ++fails;                                               \
        }                                                          \
    } while (0)

// the grammar restated: <name>:-?[0-9]{1,9}|c\n, the ':' the first one, 1 <= name <= 1425, 6 <= len <= 1449
static bool expect_parse(const std::string &s, uint32_t *k, int64_t *v) {
    if (s.size() < 6 || s.size() > 1449) return false;
    const size_t colon = s.find(':');
    if (colon == std::string::npos || colon < 1 || colon > 1425) return false;
    size_t p = colon + 1;
    bool neg = false;
    if (p < s.size() && s[p] == '-') {
        neg = true;
        ++p;
    }
    int64_t mag = 0;
    size_t nd = 0;
    while (p < s.size() && s[p] >= '0' && s[p] <= '9') {
        mag = mag * 10 + (s[p] - '0');
        ++p;
        ++nd;
    }
    if (nd < 1 || nd > 9 || s.compare(p, std::string::npos, "|c\n") != 0) return false;
    *k = (uint32_t)colon;
    *v = neg ? -mag : mag;
    return true;
}

// parse on an exact heap copy of the line
static int parse_exact(const std::string &s, uint32_t *k, int64_t *v) {
    uint8_t *line = new uint8_t[s.size() ? s.size() : 1];
    memcpy(line, s.data(), s.size());
    const int r = coalesce_parse_line(line, s.size(), k, v);
    delete[] line;
    return r;
}

static void agree(const std::string &s) {
    uint32_t k = 0, ek = 0;
    int64_t v = 0, ev = 0;
    const int got = parse_exact(s, &k, &v);
    const bool want = expect_parse(s, &ek, &ev);
    if (got != (want ? 1 : 0) || (want && (k != ek || v != ev))) {
        printf("parse disagrees on a line of %zu bytes\n", s.size());
        ++fails;
    }
}

static void format_exact(const std::string &name, int64_t sum) {
    char dec[32];
    snprintf(dec, sizeof(dec), "%lld", (long long)sum);
    const std::string want = name + ":" + dec + "|c\n";
    uint8_t *dst = new uint8_t[want.size()];   // exactly the line: one byte more written is reported
    uint8_t *src = new uint8_t[name.size() ? name.size() : 1];
    memcpy(src, name.data(), name.size());
    const size_t n = coalesce_format_line(dst, src, (uint32_t)name.size(), sum);
    CHECK(n == want.size() && memcmp(dst, want.data(), n) == 0);
    CHECK(coalesce_line_len((uint32_t)name.size(), sum) == want.size());
    // the device's form: only the bytes below `room` are written
    for (uint64_t room = 0; room <= want.size() - name.size(); ++room) {
        uint8_t *part = new uint8_t[room ? room : 1];
        CHECK(coalesce_put_tail(part, room, sum) == want.size() - name.size());
        CHECK(memcmp(part, want.data() + name.size(), room) == 0);
        delete[] part;
    }
    delete[] dst;
    delete[] src;
}

int main() {
    {   // the limits of the configuration
        uint32_t s = 0;
        sr_coalesce_config c = {0};
        CHECK(coalesce_resolve(nullptr, &s) == 0 && s == SR_COALESCE_DEFAULT_SLOTS);
        CHECK(coalesce_resolve(&c, &s) == 0 && s == 65536);
        const uint32_t bad[] = {1, 8, 15, 17, 24, 65535, SR_COALESCE_MAX_SLOTS + 1, SR_COALESCE_MAX_SLOTS * 2, 0xFFFFFFFFu};
        for (uint32_t b : bad) {
            c.slots = b;
            CHECK(coalesce_resolve(&c, &s) == -EINVAL);
        }
        for (uint32_t g = SR_COALESCE_MIN_SLOTS; g <= SR_COALESCE_MAX_SLOTS; g <<= 1) {
            c.slots = g;
            CHECK(coalesce_resolve(&c, &s) == 0 && s == g);
        }
    }
    {   // fixed lines
        uint32_t k = 0;
        int64_t v = 0;
        CHECK(parse_exact("a:1|c\n", &k, &v) == 1 && k == 1 && v == 1);
        CHECK(parse_exact("x.y:-0|c\n", &k, &v) == 1 && k == 3 && v == 0);
        CHECK(parse_exact("x.y:-999999999|c\n", &k, &v) == 1 && v == -999999999);
        CHECK(parse_exact("x.y:1234567890|c\n", &k, &v) == 0);
        CHECK(parse_exact("x:y:1|c\n", &k, &v) == 0);
        CHECK(parse_exact(std::string(1425, 'n') + ":7|c\n", &k, &v) == 1 && k == 1425 && v == 7);
        CHECK(parse_exact(std::string(1426, 'n') + ":7|c\n", &k, &v) == 0);
        CHECK(parse_exact(std::string(1450, '9'), &k, &v) == 0 && parse_exact(std::string(4096, ':'), &k, &v) == 0);
        CHECK(coalesce_parse_line(nullptr, 6, &k, &v) == 0);
        const uint8_t ok[] = {'a', ':', '1', '|', 'c', '\n'};
        CHECK(coalesce_parse_line(ok, 6, nullptr, nullptr) == 1);
    }
    {   // hostile bytes: every short line over a small alphabet by a seeded generator, and every prefix and
        // suffix of lines made of digits, '-' and ':' alone (the backward scan must stop at the line's start)
        const char alpha[] = {':', '|', 'c', '\n', '-', '+', '.', '0', '9', ' ', '\r', 'a', '\0', (char)0xFF};
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (int it = 0; it < 200000; ++it) {
            x ^= x << 13;
            x ^= x >> 7;
            x ^= x << 17;
            const size_t len = (size_t)(x % 14);
            std::string s;
            uint64_t y = x;
            for (size_t q = 0; q < len; ++q) {
                y = y * 6364136223846793005ull + 1442695040888963407ull;
                s.push_back(alpha[(y >> 33) % sizeof(alpha)]);
            }
            agree(s);
            agree(s + "|c\n");
            agree("n:" + s + "|c\n");
        }
        for (size_t len = 0; len <= 16; ++len) {
            agree(std::string(len, '7') + "|c\n");
            agree(std::string(len, '-') + "|c\n");
            agree(std::string(len, ':') + "|c\n");
            agree(std::string(len, '7'));
            agree("-" + std::string(len, '7') + "|c\n");
        }
        for (size_t len = 1400; len <= 1460; ++len) {
            agree(std::string(len, 'n') + ":1|c\n");
            agree(std::string(len, 'n') + ":-123456789|c\n");
            agree(std::string(len, 'n') + ":" + std::string(len - 1399, 'n') + ":1|c\n");
        }
    }
    {   // the merged line, at every digit count and both signs, and the clipped tail
        const int64_t sums[] = {0, 1, -1, 9, 10, -10, 99, 100, 999999999, -999999999, 1000000000, 2147483648ll, -2147483648ll,
                                (1ll << 60) - 1, -(1ll << 60), INT64_MAX, INT64_MIN, 1000000000000000000ll, 999999999999999999ll};
        for (int64_t s : sums) {
            format_exact("a", s);
            format_exact("svc.req.count", s);
            format_exact(std::string(1425, 'n'), s);
            format_exact(std::string("n\0\xff", 3), s);
        }
        int64_t p = 1;
        for (int d = 1; d <= 18; ++d, p *= 10) {
            CHECK(coalesce_dec_len(p) == (uint32_t)d && coalesce_dec_len(-p) == (uint32_t)d + 1);
            CHECK(coalesce_dec_len(p * 10 - 1) == (uint32_t)d);
        }
        CHECK(coalesce_dec_len(INT64_MIN) == 20 && coalesce_dec_len(0) == 1);
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
