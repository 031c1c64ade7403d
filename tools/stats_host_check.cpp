// stats_host_check.cpp — the snapshot functions of the name statistics (statsd-router_amd/csrc/stats_host.hpp)
// in a stand-alone host program, meant for -fsanitize=address,undefined (tests/test_stats_host_check.py): every
// snapshot is one heap block of exactly its stated size, so a register, cell or hot entry touched past its
// array is reported. Prints "ok".
#include <stdio.h>

#include <map>
#include <vector>

#include "../statsd-router_amd/csrc/stats_host.hpp"

using namespace srk;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("line %d: %s\n", __LINE__, #c);                 \
            ++fails;                                               \
        }                                                          \
    } while (0)

// the restated update of one valid line (include/sr_route.h), on a host snapshot
static void count_line(sr_stats_snapshot *s, const char *name, uint32_t shard, uint32_t bytes) {
    const uint64_t h = stats_name_hash((const uint8_t *)name, strlen(name)), m = stats_fmix64(h);
    const uint32_t p = s->cfg.hll_p;
    s->lines[0]++;
    s->bytes[0] += bytes;
    s->shard_lines[shard]++;
    s->shard_bytes[shard] += bytes;
    const uint64_t w = m << p;
    const uint8_t rho = (uint8_t)(w ? __builtin_clzll(w) + 1 : 64 - p + 1);
    uint8_t &reg = s->regs[((size_t)shard << p) + (m >> (64 - p))];
    if (reg < rho) reg = rho;
    for (uint32_t r = 0; r < s->cfg.cms_rows; ++r) s->cells[(size_t)r * s->cfg.cms_width + stats_cell(m, r, s->cfg.cms_width - 1)]++;
}

static void add_hot(sr_stats_snapshot *s, const char *name) {
    sr_stats_hot &e = s->hot[s->n_hot++];
    memset(&e, 0, sizeof(e));
    e.hash = stats_name_hash((const uint8_t *)name, strlen(name));
    e.name_len = (uint32_t)strlen(name);
    memcpy(e.name, name, e.name_len < SR_STATS_NAME_MAX ? e.name_len : SR_STATS_NAME_MAX);
}

int main() {
    static_assert(sizeof(sr_stats_hot) == 128, "hot entry");
    CHECK(stats_fmix64(0) == 0 && stats_fmix64(1) != 1);
    {   // sdbm with signed char, against the reference's loop
        const uint8_t b[] = {0x80, 0xFF, 'a', 0x00, 0x7F, 0xC3, 0xA9};
        unsigned long h = 0;
        for (size_t i = 0; i < sizeof(b); ++i) h = (h << 6) + (h << 16) - h + (unsigned long)(long)(signed char)b[i];
        CHECK(stats_name_hash(b, sizeof(b)) == (uint64_t)h && stats_name_hash(b, 0) == 0);
    }
    {   // defaults and every limit
        sr_stats_config z = {0, 0, 0, 0, 0, 0}, o;
        CHECK(stats_resolve(&z, 4, &o) == 0 && o.hll_p == 10 && o.cms_rows == 4 && o.cms_width == 4096 && o.hot_slots == 256 &&
              o.hot_div == 256 && o.hot_min_lines == 1024);
        CHECK(stats_resolve(nullptr, 4, &o) == 0);
        const sr_stats_config good = {4, 8, 2048, 4096, 1, 0};
        CHECK(stats_resolve(&good, 65533, &o) == 0);
        const sr_stats_config bad[] = {{3, 1, 256, 4, 1, 0}, {13, 1, 256, 4, 1, 0}, {11, 1, 256, 4, 1, 0}, {4, 0, 256, 4, 1, 0},
                                       {4, 9, 256, 4, 1, 0}, {4, 1, 128, 4, 1, 0}, {4, 1, 384, 4, 1, 0}, {4, 8, 4096, 4, 1, 0},
                                       {4, 1, 256, 2, 1, 0}, {4, 1, 256, 8192, 1, 0}, {4, 1, 256, 6, 1, 0}, {4, 1, 256, 4, 0, 0}};
        for (const sr_stats_config &c : bad) CHECK(stats_resolve(&c, 65533, &o) == -EINVAL);
    }
    const sr_stats_config cfg = {6, 3, 256, 4, 8, 2};
    const uint32_t nds = 5;
    sr_stats_snapshot *a = stats_snap_alloc(cfg, nds), *b = stats_snap_alloc(cfg, nds);
    CHECK(a && b && stats_snap_ok(a));
    std::map<uint64_t, uint64_t> truth;
    char name[64];
    for (int i = 0; i < 3000; ++i) {
        snprintf(name, sizeof(name), "svc.req.%d", (i * 7919) % 700);
        count_line(i & 1 ? a : b, name, (uint32_t)(i % nds), 20);
        truth[stats_name_hash((const uint8_t *)name, strlen(name))]++;
    }
    for (int i = 0; i < 500; ++i) count_line(a, "hot.one", 1, 11), count_line(b, "hot.two", 2, 13);
    truth[stats_name_hash((const uint8_t *)"hot.one", 7)] += 500;
    truth[stats_name_hash((const uint8_t *)"hot.two", 7)] += 500;
    add_hot(a, "hot.one");
    add_hot(a, "svc.req.1");
    add_hot(b, "hot.two");
    add_hot(b, "svc.req.1");
    add_hot(b, "svc.req.2");
    stats_sort_hot(a);
    stats_sort_hot(b);
    const uint64_t cell0 = a->cells[0] + b->cells[0];
    const double ca = stats_cardinality(a, SR_STATS_ALL), cb = stats_cardinality(b, SR_STATS_ALL);
    CHECK(stats_merge(a, b) == 0);
    CHECK(a->lines[0] == 4000 && a->bytes[0] == 3000 * 20 + 500 * 24 && a->cells[0] == cell0);
    CHECK(a->n_hot == 4 && !a->hot_overflow);   // the union: hot.one, hot.two, svc.req.1, svc.req.2
    for (uint32_t i = 0; i + 1 < a->n_hot; ++i) {
        CHECK(a->hot[i].lines > a->hot[i + 1].lines || (a->hot[i].lines == a->hot[i + 1].lines && a->hot[i].hash < a->hot[i + 1].hash));
        CHECK(a->hot[i].lines == stats_estimate(a, a->hot[i].hash));
    }
    for (const auto &t : truth) CHECK(stats_estimate(a, t.first) >= t.second);   // never under
    const double all = stats_cardinality(a, SR_STATS_ALL);
    CHECK(all >= ca && all >= cb && all > 702 * (1 - 4 * 1.04 / 8) && all < 702 * (1 + 4 * 1.04 / 8));   // m = 64
    double parts = 0;
    for (uint32_t k = 0; k < nds; ++k) parts += stats_cardinality(a, k);
    CHECK(parts > 0);
    // a fifth distinct hot name does not fit four slots
    sr_stats_snapshot *c = stats_snap_alloc(cfg, nds);
    add_hot(c, "svc.req.3");
    CHECK(stats_merge(a, c) == 0 && a->n_hot == 4 && a->hot_overflow == 1);
    // mismatches are refused and change nothing
    const sr_stats_config other = {6, 3, 512, 4, 8, 2};
    sr_stats_snapshot *d = stats_snap_alloc(other, nds), *e = stats_snap_alloc(cfg, nds + 1);
    CHECK(stats_merge(a, d) == -EINVAL && stats_merge(a, e) == -EINVAL && a->lines[0] == 4000);
    // m = 16 / 32 / 64 alphas and the empty sketch
    for (uint32_t p = 4; p <= 12; ++p) {
        const sr_stats_config pc = {p, 1, 256, 4, 1, 0};
        sr_stats_snapshot *s = stats_snap_alloc(pc, 2);
        CHECK(stats_cardinality(s, SR_STATS_ALL) == 0.0 && stats_cardinality(s, 1) == 0.0);
        for (int i = 0; i < 2000; ++i) {
            snprintf(name, sizeof(name), "test.counter%d", i);
            count_line(s, name, (uint32_t)(i & 1), 1);
        }
        const double est = stats_cardinality(s, SR_STATS_ALL), bound = 4 * 1.04 / sqrt((double)(1u << p));
        CHECK(est > 2000 * (1 - bound) && est < 2000 * (1 + bound));
        free(s);
    }
    free(a), free(b), free(c), free(d), free(e);
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
