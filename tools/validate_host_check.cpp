// validate_host_check.cpp — the host part of the line grammar (statsd-router_amd/csrc/validate_host.hpp) in a
// stand-alone host program, meant for -fsanitize=address,undefined (tests/test_validate_host_check.py): every line
// is a heap block of exactly its size, so a byte read past its end or before its start is reported. Lines with
// known reasons, every truncation of them, every single-byte mutation of them (compared with a plain byte-by-byte
// judge written here from the contract), the configurations, the names and the specs. Prints "ok".
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../statsd-router_amd/csrc/validate_host.hpp"

using namespace srk;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("line %d: %s\n", __LINE__, #c);                 \
            ++fails;                                               \
        }                                                          \
    } while (0)

static bool is_tb(uint8_t b) { return b >= 0x21 && b <= 0x7E && b != '|'; }

static bool is_number(const std::string &s) {
    size_t i = 0, d = 0;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') ++i, ++d;
    if (d < 1 || d > 20) return false;
    if (i == s.size()) return true;
    if (s[i] != '.') return false;
    ++i;
    d = 0;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') ++i, ++d;
    return d >= 1 && d <= 20 && i == s.size();
}

// the contract, field by field
static uint32_t plain(const std::string &line, uint32_t accept) {
    std::string c = line;
    if (!c.empty() && c.back() == '\n') c.pop_back();
    const size_t p = c.find(':');
    if (p == std::string::npos) return SR_VALID_NO_COLON;
    if (p == 0) return SR_VALID_EMPTY_NAME;
    for (size_t i = 0; i < p; ++i)
        if (!is_tb((uint8_t)c[i])) return SR_VALID_NAME_BYTE;   // no ':' before p
    std::vector<std::string> f(1);
    for (size_t i = p + 1; i < c.size(); ++i) {
        if (c[i] == '|') f.emplace_back();
        else f.back().push_back(c[i]);
    }
    if (f.size() == 1) return SR_VALID_NO_TYPE;
    const std::string &t = f[1];
    const uint32_t bit = t == "c" ? SR_VALID_TYPE_C : t == "g" ? SR_VALID_TYPE_G : t == "ms" ? SR_VALID_TYPE_MS
                       : t == "h" ? SR_VALID_TYPE_H : t == "s" ? SR_VALID_TYPE_S : t == "d" ? SR_VALID_TYPE_D : 0u;
    if (!(bit & accept)) return SR_VALID_TYPE;
    std::string v = f[0];
    bool ok;
    if (bit == SR_VALID_TYPE_S) {
        ok = v.size() >= 1 && v.size() <= 64;
        for (char ch : v) ok = ok && is_tb((uint8_t)ch);
    } else {
        if (!v.empty() && (v[0] == '-' || (v[0] == '+' && bit == SR_VALID_TYPE_G)) && (bit == SR_VALID_TYPE_C || bit == SR_VALID_TYPE_G))
            v.erase(0, 1);
        ok = is_number(v);
    }
    if (!ok) return SR_VALID_VALUE;
    bool at = false, hash = false;
    for (size_t k = 2; k < f.size(); ++k) {
        const std::string &x = f[k];
        if (x.empty() || (x[0] != '@' && x[0] != '#')) return SR_VALID_SECTION;
        if (x[0] == '@') {
            if (at || hash) return SR_VALID_SECTION;
            at = true;
            if (!is_number(x.substr(1)) || bit == SR_VALID_TYPE_G || bit == SR_VALID_TYPE_S) return SR_VALID_RATE;
        } else {
            if (hash) return SR_VALID_SECTION;
            hash = true;
            if (x.size() < 2) return SR_VALID_TAGS;
            for (size_t i = 1; i < x.size(); ++i)
                if (!is_tb((uint8_t)x[i])) return SR_VALID_TAGS;
        }
    }
    return SR_VALID_OK;
}

// the shared judgement over a heap block of exactly the line's size
static uint32_t judged(const std::string &line, uint32_t accept) {
    uint8_t *p = new uint8_t[line.size()];
    memcpy(p, line.data(), line.size());
    const uint32_t r = validate_line(p, line.size(), accept);
    delete[] p;
    return r;
}

int main() {
    struct Known {
        const char *text;
        uint32_t reason;
    };
    const Known known[] = {
        {"a:1|c\n", SR_VALID_OK}, {"a:x", SR_VALID_NO_TYPE}, {"a:x|q", SR_VALID_TYPE}, {"a:1|g|@0.5", SR_VALID_RATE},
        {"a:1|c|#t|@1", SR_VALID_SECTION}, {"a:1|c|@1|@1", SR_VALID_SECTION}, {"abc\n", SR_VALID_NO_COLON},
        {":1|c\n", SR_VALID_EMPTY_NAME}, {"a b:1|c\n", SR_VALID_NAME_BYTE}, {"a:|c\n", SR_VALID_VALUE},
        {"a:1|c|#\n", SR_VALID_TAGS}, {"\n", SR_VALID_NO_COLON}, {"a:+1|c\n", SR_VALID_VALUE}, {"a:+1|g\n", SR_VALID_OK},
        {"a:-1|ms\n", SR_VALID_VALUE}, {"a:b:c|s|#x:y\n", SR_VALID_OK}, {"a:1|c|", SR_VALID_SECTION},
    };
    for (const Known &k : known) {
        CHECK(judged(k.text, kValidTypesAll) == k.reason);
        CHECK(plain(k.text, kValidTypesAll) == k.reason);
    }
    const std::vector<std::string> seeds = {
        "svc.req:1|c\n",
        "svc.req.count:12.5|ms|@0.25\n",
        "a.b:-3.25|c|@1|#env:prod,zone:a\n",
        "gauge.x:+17|g|#t\n",
        "users.uniq:alice:bob|s\n",
        "lat:00000000000000000020.00000000000000000020|h|@0.1|#k:v\n",
        "dist.v:7|d|@0.5\n",
        "n:0|g",
        "a-very.long_name/with~bytes:18446744073709551615|c|#a,b,c\n",
        std::string("a:") + std::string(64, 'v') + "|s|#" + std::string(200, 't') + "\n",
    };
    size_t n = 0;
    for (const std::string &s : seeds) {
        CHECK(judged(s, kValidTypesAll) == SR_VALID_OK);
        for (size_t k = 1; k <= s.size(); ++k) {
            const std::string cut = s.substr(0, k);
            CHECK(judged(cut, kValidTypesAll) == plain(cut, kValidTypesAll));
            ++n;
        }
        for (size_t at = 0; at < s.size(); ++at)
            for (int v = 0; v < 256; ++v) {
                std::string m = s;
                m[at] = (char)v;
                const uint32_t a = judged(m, kValidTypesAll), b = plain(m, kValidTypesAll);
                if (a != b) {
                    printf("mutation at %zu to %d of seed '%s': %u, want %u\n", at, v, s.c_str(), a, b);
                    ++fails;
                }
                ++n;
            }
        for (uint32_t types : {1u, 6u, 47u, 32u}) CHECK(judged(s, types) == plain(s, types));
    }
    CHECK(n > 60000);
    // lines of every length around the steps, name only and tags only
    for (size_t len = 1; len <= 70; ++len) {
        const std::string name(len, 'n');
        CHECK(judged(name, kValidTypesAll) == SR_VALID_NO_COLON);
        CHECK(judged(name + ":1|c", kValidTypesAll) == SR_VALID_OK);
        CHECK(judged("a:1|c|#" + std::string(len, 't'), kValidTypesAll) == SR_VALID_OK);
        CHECK(judged("a:1|c|#" + std::string(len, 't') + "\n", kValidTypesAll) == SR_VALID_OK);
        CHECK(judged("a:1|c|#" + std::string(len, 't') + " ", kValidTypesAll) == SR_VALID_TAGS);
    }
    CHECK(judged(std::string(1449, 'n'), kValidTypesAll) == SR_VALID_NO_COLON);
    CHECK(judged("a:1|c|#" + std::string(1441, 't') + "\n", kValidTypesAll) == SR_VALID_OK);

    // configurations
    sr_validate_config cfg = {0u, kValidTypesAll};
    CHECK(validate_check(&cfg) == 0);
    CHECK(validate_check(nullptr) == -EINVAL);
    cfg.drop_mask = 1u;
    CHECK(validate_check(&cfg) == -EINVAL);
    cfg.drop_mask = 1u << SR_VALID_REASONS;
    CHECK(validate_check(&cfg) == -EINVAL);
    cfg.drop_mask = kValidDropAll;
    CHECK(validate_check(&cfg) == 0);
    cfg.accept_types = 0u;
    CHECK(validate_check(&cfg) == -EINVAL);
    cfg.accept_types = 64u;
    CHECK(validate_check(&cfg) == -EINVAL);

    // names and specs; a spec is a heap block of exactly its size with its NUL
    CHECK(validate_reason_name(SR_VALID_REASONS) == nullptr);
    const char *good[] = {"count", "drop", "value", "value,tags", "no_colon,empty_name,name_byte,no_type,type,value,section,rate,tags"};
    const uint32_t masks[] = {0u, kValidDropAll, 1u << SR_VALID_VALUE, (1u << SR_VALID_VALUE) | (1u << SR_VALID_TAGS), kValidDropAll};
    for (size_t i = 0; i < sizeof(good) / sizeof(good[0]); ++i) {
        char *t = new char[strlen(good[i]) + 1];
        strcpy(t, good[i]);
        sr_validate_config out = {77u, 77u};
        CHECK(validate_parse_spec(t, &out) == 0 && out.drop_mask == masks[i] && out.accept_types == kValidTypesAll);
        delete[] t;
    }
    const char *bad[] = {"", "ok", "value,", ",value", "Value", "drop,count", "valu", "values", " drop"};
    for (const char *b : bad) {
        char *t = new char[strlen(b) + 1];
        strcpy(t, b);
        sr_validate_config out = {77u, 77u};
        CHECK(validate_parse_spec(t, &out) == -EINVAL && out.drop_mask == 77u);
        delete[] t;
    }
    CHECK(validate_parse_spec(nullptr, &cfg) == -EINVAL);
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
