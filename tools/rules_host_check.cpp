// rules_host_check.cpp — the host part of the name rules (statsd-router_amd/csrc/rules_host.hpp) in a stand-alone
// host program, meant for -fsanitize=address,undefined (tests/test_rules_host_check.py): every line, every pattern,
// every rule file and every compiled table is a heap block of exactly its size, so a byte read or written past any
// of them is reported. The matcher is compared with a brute-force longest match over all rules. Prints "ok".
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../statsd-router_amd/csrc/rules_host.hpp"

using namespace srk;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("line %d: %s\n", __LINE__, #c);                 \
            ++fails;                                               \
        }                                                          \
    } while (0)

struct Rule {
    std::string text;
    uint8_t kind, action;
};

// a rule set whose patterns are heap blocks of exactly their lengths
struct Set {
    std::vector<uint8_t *> blocks;
    std::vector<sr_rule> rules;
    sr_rules_config cfg;
    Set(const std::vector<Rule> &in, uint32_t default_action) {
        for (const Rule &r : in) {
            uint8_t *p = new uint8_t[r.text.size() ? r.text.size() : 1];
            memcpy(p, r.text.data(), r.text.size());
            blocks.push_back(p);
            rules.push_back(sr_rule{p, (uint32_t)r.text.size(), r.kind, r.action});
        }
        cfg.rules = rules.data();
        cfg.n_rules = (uint32_t)rules.size();
        cfg.default_action = default_action;
    }
    ~Set() {
        for (uint8_t *p : blocks) delete[] p;
    }
};

// the header's definition, every rule tried
static uint32_t brute(const std::vector<Rule> &rules, const std::string &line) {
    uint32_t best = (uint32_t)rules.size();
    size_t best_len = 0;
    int best_kind = -1;
    const size_t L = line.size();
    for (size_t i = 0; i < rules.size(); ++i) {
        const std::string &p = rules[i].text;
        bool m;
        if (rules[i].kind == SR_RULE_PREFIX) m = p.size() + 1 <= L && line.compare(0, p.size(), p) == 0;
        else m = p.size() + 2 <= L && line.compare(0, p.size(), p) == 0 && line[p.size()] == ':';
        if (m && (best_kind < 0 || p.size() > best_len || (p.size() == best_len && rules[i].kind > best_kind))) {
            best = (uint32_t)i;
            best_len = p.size();
            best_kind = rules[i].kind;
        }
    }
    return best;
}

static uint32_t match_exact(const RulesTable *t, const std::string &s) {
    uint8_t *line = new uint8_t[s.size() ? s.size() : 1];
    memcpy(line, s.data(), s.size());
    const uint32_t r = rules_match(*t, line, s.size());
    delete[] line;
    return r;
}

static uint32_t rnd_state = 12345u;
static uint32_t rnd(uint32_t n) {
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return (rnd_state >> 8) % n;
}

static std::string rnd_text(size_t n, const char *alphabet, size_t na) {
    std::string s;
    for (size_t i = 0; i < n; ++i) s.push_back(alphabet[rnd((uint32_t)na)]);
    return s;
}

static void check_sets() {
    CHECK(rules_check_shape(nullptr) == -EINVAL);
    RulesTable *t = new RulesTable;
    {
        Set s({}, SR_RULE_KEEP);
        CHECK(rules_compile(&s.cfg, t) == 0 && t->n_entries == 0 && t->n_rules == 0);
        CHECK(match_exact(t, "a:1|c\n") == 0 && match_exact(t, "") == 0);
    }
    {
        Set s({{"", SR_RULE_PREFIX, SR_RULE_DROP}}, SR_RULE_KEEP);
        CHECK(rules_compile(&s.cfg, t) == -EINVAL);
    }
    {
        Set s({{std::string(65, 'x'), SR_RULE_PREFIX, SR_RULE_DROP}}, SR_RULE_KEEP);
        CHECK(rules_compile(&s.cfg, t) == -EINVAL);
    }
    {
        Set a({{"a:b", SR_RULE_PREFIX, SR_RULE_DROP}}, SR_RULE_KEEP), b({{"a\nb", SR_RULE_EXACT, SR_RULE_DROP}}, SR_RULE_KEEP);
        CHECK(rules_compile(&a.cfg, t) == -EINVAL && rules_compile(&b.cfg, t) == -EINVAL);
    }
    {
        Set s({{"ab", SR_RULE_PREFIX, SR_RULE_DROP}, {"c", SR_RULE_PREFIX, SR_RULE_DROP}, {"ab", SR_RULE_PREFIX, SR_RULE_KEEP}},
              SR_RULE_KEEP);
        CHECK(rules_compile(&s.cfg, t) == -EINVAL);
        Set ok({{"ab", SR_RULE_PREFIX, SR_RULE_DROP}, {"ab", SR_RULE_EXACT, SR_RULE_KEEP}}, 2);
        CHECK(rules_compile(&ok.cfg, t) == -EINVAL);   // the default action
    }
    {
        std::vector<Rule> many;
        for (int i = 0; i < 257; ++i) many.push_back({"r" + std::to_string(1000 + i), SR_RULE_PREFIX, SR_RULE_DROP});
        Set s(many, SR_RULE_KEEP);
        CHECK(rules_compile(&s.cfg, t) == -EINVAL);
        many.pop_back();
        Set s2(many, SR_RULE_KEEP);
        CHECK(rules_compile(&s2.cfg, t) == 0 && t->n_entries == 256);
    }
    {
        std::vector<Rule> full;   // 64 x 64 bytes = 4096: the whole text, and the last pattern ends the block
        for (int i = 0; i < 64; ++i) full.push_back({std::to_string(10 + i) + std::string(62, 'y'), SR_RULE_EXACT, SR_RULE_DROP});
        Set s(full, SR_RULE_KEEP);
        CHECK(rules_compile(&s.cfg, t) == 0);
        for (int i = 0; i < 64; ++i) {
            CHECK(match_exact(t, full[i].text + ":1|c\n") == (uint32_t)i);
            CHECK(match_exact(t, full[i].text + ":") == 64u);
            CHECK(match_exact(t, full[i].text) == 64u);
        }
        full.push_back({"z", SR_RULE_EXACT, SR_RULE_DROP});
        Set s2(full, SR_RULE_KEEP);
        CHECK(rules_compile(&s2.cfg, t) == -EINVAL);
    }
    delete t;
}

static void check_matches() {
    static const char alphabet[] = {'a', 'b', '.', '\0', (char)0xFF};
    static const char line_alphabet[] = {'a', 'b', '.', '\0', (char)0xFF, ':', '\n'};
    for (int round = 0; round < 60; ++round) {
        std::vector<Rule> rules;
        std::vector<std::string> texts{rnd_text(1 + rnd(3), alphabet, sizeof(alphabet))};
        const size_t want = 1 + rnd(round < 50 ? 40 : 256);
        size_t bytes = 0;
        for (int tries = 0; rules.size() < want && tries < 4000; ++tries) {
            std::string t = texts[rnd((uint32_t)texts.size())] + rnd_text(rnd(round % 3 ? 12 : 40), alphabet, sizeof(alphabet));
            if (t.size() > 64) t.resize(64);
            const uint8_t kind = (uint8_t)rnd(2);
            bool dup = false;
            for (const Rule &r : rules) dup = dup || (r.kind == kind && r.text == t);
            if (dup || bytes + t.size() > 4096) continue;
            bytes += t.size();
            texts.push_back(t);
            rules.push_back({t, kind, (uint8_t)rnd(2)});
        }
        Set s(rules, SR_RULE_KEEP);
        RulesTable *t = new RulesTable;   // a heap block of exactly the table
        CHECK(rules_compile(&s.cfg, t) == 0);
        for (int k = 0; k < 800; ++k) {
            const std::string &base = texts[rnd((uint32_t)texts.size())];
            std::string line = base.substr(0, rnd((uint32_t)base.size() + 1)) + rnd_text(rnd(10), line_alphabet, sizeof(line_alphabet));
            if (rnd(4)) line.push_back('\n');
            const uint32_t got = match_exact(t, line), exp = brute(rules, line);
            if (got != exp) {
                printf("round %d: a line of %zu bytes: got rule %u, want %u\n", round, line.size(), got, exp);
                ++fails;
            }
        }
        // every pattern as a line's whole head, with each byte behind it
        for (const Rule &r : rules)
            for (const char *tail : {"", ":", "\n", ":\n", "x\n", ":1|c\n"})
                if (match_exact(t, r.text + tail) != brute(rules, r.text + tail)) {
                    printf("round %d: a pattern of %zu bytes with a tail of %zu\n", round, r.text.size(), strlen(tail));
                    ++fails;
                }
        delete t;
    }
}

// the rule file on a heap block of exactly its length
static int parse_exact(const std::string &text, sr_rules_config **out, size_t *line) {
    char *p = new char[text.size() ? text.size() : 1];
    memcpy(p, text.data(), text.size());
    const int rc = rules_parse_text(p, text.size(), out, line);
    delete[] p;
    return rc;
}

static void check_files() {
    sr_rules_config *cfg = nullptr;
    size_t line = 99;
    CHECK(parse_exact("# c\n\ndrop debug.*\nkeep debug.keep.*\ndrop app.x\ndefault drop", &cfg, &line) == 0 && line == 0);
    if (cfg) {
        CHECK(cfg->n_rules == 3 && cfg->default_action == SR_RULE_DROP);
        CHECK(cfg->rules[0].kind == SR_RULE_PREFIX && cfg->rules[0].len == 6 && memcmp(cfg->rules[0].pattern, "debug.", 6) == 0);
        CHECK(cfg->rules[2].kind == SR_RULE_EXACT && cfg->rules[2].action == SR_RULE_DROP && cfg->rules[2].len == 5);
        free(cfg);
    }
    CHECK(parse_exact("", &cfg, &line) == 0 && cfg && cfg->n_rules == 0 && cfg->default_action == SR_RULE_KEEP);
    free(cfg);
    CHECK(parse_exact("drop", &cfg, &line) == -EINVAL && line == 1 && !cfg);
    CHECK(parse_exact("drop ", &cfg, &line) == -EINVAL && line == 1);
    CHECK(parse_exact("drop *", &cfg, &line) == -EINVAL && line == 1);
    CHECK(parse_exact("keep a\nmute b", &cfg, &line) == -EINVAL && line == 2);
    CHECK(parse_exact("keep a\n\n# x\nkeep a\n", &cfg, &line) == -EINVAL && line == 4);
    CHECK(parse_exact("default", &cfg, &line) == -EINVAL && line == 1);
    CHECK(parse_exact("default drop\ndefault drop\n", &cfg, &line) == -EINVAL && line == 2);
    CHECK(parse_exact("drop a:b\n", &cfg, &line) == -EINVAL && line == 1);
    CHECK(parse_exact("drop " + std::string(65, 'x'), &cfg, &line) == -EINVAL && line == 1);
    CHECK(parse_exact("drop " + std::string(64, 'x') + "*", &cfg, &line) == 0 && cfg && cfg->rules[0].len == 64);
    free(cfg);
    std::string many;
    for (int i = 0; i < 257; ++i) many += "drop r" + std::to_string(1000 + i) + "\n";
    CHECK(parse_exact(many, &cfg, &line) == -EINVAL && line == 257);
    for (int k = 0; k < 2000; ++k) {   // hostile files: they parse or they do not, within their bytes
        static const char fa[] = {'d', 'r', 'o', 'p', 'k', 'e', ' ', '*', '\n', '#', ':', 'a', '\0'};
        const std::string text = (rnd(2) ? "drop " : "") + rnd_text(rnd(40), fa, sizeof(fa));
        if (parse_exact(text, &cfg, &line) == 0) free(cfg);
    }
}

int main() {
    check_sets();
    check_matches();
    check_files();
    if (fails) {
        printf("%d failures\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
