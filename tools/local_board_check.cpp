// local_board_check.cpp — the rendezvous board of the in-process communicator on the CPU.
//
// Includes only statsd-router_amd/csrc/local_board.hpp; the device is a fake (events are flags, the pull
// is memcpy). Ranks are threads. Built and run by tests/test_local_board.py with plain g++; the same
// program is meant for -fsanitize=thread and -fsanitize=address,undefined builds:
//   g++ -std=c++17 -O1 -g -pthread [-fsanitize=thread] -o local_board_check tools/local_board_check.cpp
// Exit status 0 and "ok" on stdout: every check passed.
#include "../statsd-router_amd/csrc/local_board.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace srk;

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

struct FakeEvent {
    std::atomic<int> recorded{0};
};

// A rank's device: events of a ring, recorded before anyone else sees them; the pull copies at once.
struct FakeDev {
    FakeEvent ring[8];
    unsigned next = 0;
    size_t pulls = 0, pulled_bytes = 0, waits = 0;
    int record(void **ev) {
        FakeEvent *e = &ring[next++ % 8];
        e->recorded.store(1, std::memory_order_release);
        *ev = e;
        return 0;
    }
    int wait(void *ev) {
        CHECK(ev && ((FakeEvent *)ev)->recorded.load(std::memory_order_acquire) == 1);   // the invariant
        ++waits;
        return 0;
    }
    int pull(const BoardSeg *segs, size_t n) {
        ++pulls;
        for (size_t i = 0; i < n; ++i) {
            memcpy(segs[i].dst, segs[i].src, segs[i].bytes);
            pulled_bytes += segs[i].bytes;
        }
        return 0;
    }
};

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the byte k of message (round, src, dst, tag, j)
static uint8_t pattern(int round, int src, int dst, int tag, int j, size_t k) {
    return (uint8_t)(round * 131 + src * 31 + dst * 17 + tag * 7 + j * 3 + (int)k);
}
static size_t msg_bytes(int round, int src, int dst, int tag, int j) {
    return 1 + (size_t)((round * 7 + src * 5 + dst * 3 + tag * 11 + j) % 61);
}

// `world` threads, `rounds` groups each: to and from every peer two messages under tag 0 (their order
// must hold) and one under tags 1 and 2, sizes and bytes telling (round, source, tag, index) apart.
static void all_pairs(int world, int rounds) {
    LocalBoard board(world);
    std::vector<FakeDev> devs((size_t)world);   // outlive the threads: a peer may still wait for a rank's last event
    std::vector<std::thread> th;
    for (int r = 0; r < world; ++r)
        th.emplace_back([&, r] {
            FakeDev &dev = devs[(size_t)r];
            const int per_peer = 4;
            const int tags[per_peer] = {0, 0, 1, 2}, idx[per_peer] = {0, 1, 0, 0};
            std::vector<std::vector<uint8_t>> out((size_t)world * per_peer), in((size_t)world * per_peer);
            for (int round = 0; round < rounds; ++round) {
                std::vector<BoardOp> ops;
                for (int q = 0; q < world; ++q) {
                    if (q == r) continue;
                    for (int m = 0; m < per_peer; ++m) {
                        std::vector<uint8_t> &o = out[(size_t)q * per_peer + m], &i = in[(size_t)q * per_peer + m];
                        o.resize(msg_bytes(round, r, q, tags[m], idx[m]));
                        for (size_t k = 0; k < o.size(); ++k) o[k] = pattern(round, r, q, tags[m], idx[m], k);
                        i.assign(msg_bytes(round, q, r, tags[m], idx[m]), 0xEE);
                        ops.push_back(BoardOp{true, q, tags[m], o.data(), o.size()});
                        ops.push_back(BoardOp{false, q, tags[m], i.data(), i.size()});
                    }
                }
                CHECK(board.run_group(r, ops, nullptr, 0, dev, 60000) == 0);
                for (int q = 0; q < world; ++q) {
                    if (q == r) continue;
                    for (int m = 0; m < per_peer; ++m) {
                        const std::vector<uint8_t> &i = in[(size_t)q * per_peer + m];
                        for (size_t k = 0; k < i.size(); ++k) CHECK(i[k] == pattern(round, q, r, tags[m], idx[m], k));
                    }
                }
            }
            CHECK(dev.pulls == (size_t)rounds);   // one pull per group
        });
    for (std::thread &t : th) t.join();
    CHECK(!board.broken());
}

// A rank without operations returns at once (its peers never call), with and without a deadline; a copy
// within the rank alone needs no peer either.
static void idle_rank() {
    LocalBoard board(3);
    FakeDev dev;
    std::vector<BoardOp> none;
    const auto t0 = std::chrono::steady_clock::now();
    CHECK(board.run_group(2, none, nullptr, 0, dev, 0) == 0);
    CHECK(board.run_group(2, none, nullptr, 0, dev, 50) == 0);
    uint8_t a[5] = {1, 2, 3, 4, 5}, b[5] = {0};
    const BoardSeg own{a, b, 5};
    CHECK(board.run_group(1, none, &own, 1, dev, 0) == 0);
    CHECK(memcmp(a, b, 5) == 0 && dev.pulls == 1 && dev.waits == 0);
    CHECK(ms_since(t0) < 1000.0);
    CHECK(board.run_group(3, none, nullptr, 0, dev, 0) == -EINVAL);
    std::vector<BoardOp> self{BoardOp{true, 1, 0, a, 5}};
    CHECK(board.run_group(1, self, nullptr, 0, dev, 0) == -EINVAL);   // a send to itself
    std::vector<BoardOp> tag{BoardOp{true, 0, kBoardTags, a, 5}};
    CHECK(board.run_group(1, tag, nullptr, 0, dev, 0) == -EINVAL);
    CHECK(!board.broken());
}

// A receive of 8 bytes against a send of 16: -EMSGSIZE at the receiver, nothing copied, the board broken
// (the sender is woken with -EPIPE), every later group -EPIPE.
static void size_mismatch() {
    LocalBoard board(2);
    uint8_t src[16], dst[16];
    memset(src, 0x11, sizeof(src));
    memset(dst, 0xCD, sizeof(dst));
    int rc0 = 0, rc1 = 0;
    std::thread t0([&] {
        FakeDev dev;
        std::vector<BoardOp> ops{BoardOp{true, 1, 1, src, 16}};
        rc0 = board.run_group(0, ops, nullptr, 0, dev, 60000);
    });
    std::thread t1([&] {
        FakeDev dev;
        std::vector<BoardOp> ops{BoardOp{false, 0, 1, dst, 8}};
        rc1 = board.run_group(1, ops, nullptr, 0, dev, 60000);
        CHECK(dev.pulls == 0);
    });
    t0.join();
    t1.join();
    CHECK(rc1 == -EMSGSIZE && rc0 == -EPIPE && board.broken());
    for (uint8_t b : dst) CHECK(b == 0xCD);
    FakeDev dev;
    std::vector<BoardOp> ops{BoardOp{true, 1, 0, src, 16}};
    CHECK(board.run_group(0, ops, nullptr, 0, dev, 0) == -EPIPE);
}

// An absent peer: -ETIMEDOUT after the deadline and not before; the latecomer gets -EPIPE at once.
static void absent_peer() {
    LocalBoard board(2);
    uint8_t a[8] = {0}, b[8] = {0};
    FakeDev dev0, dev1;
    std::vector<BoardOp> ops0{BoardOp{true, 1, 0, a, 8}, BoardOp{false, 1, 0, b, 8}};
    auto t0 = std::chrono::steady_clock::now();
    CHECK(board.run_group(0, ops0, nullptr, 0, dev0, 150) == -ETIMEDOUT);
    const double waited = ms_since(t0);
    CHECK(waited >= 150.0 && waited < 5000.0);
    CHECK(board.broken() && dev0.pulls == 0);
    std::vector<BoardOp> ops1{BoardOp{true, 0, 0, b, 8}, BoardOp{false, 0, 0, a, 8}};
    t0 = std::chrono::steady_clock::now();
    CHECK(board.run_group(1, ops1, nullptr, 0, dev1, 60000) == -EPIPE);
    CHECK(ms_since(t0) < 1000.0 && dev1.pulls == 0);
    // a sender whose message is never pulled times out the same way
    LocalBoard b2(2);
    std::vector<BoardOp> only_send{BoardOp{true, 1, 2, a, 8}};
    t0 = std::chrono::steady_clock::now();
    CHECK(b2.run_group(0, only_send, nullptr, 0, dev0, 100) == -ETIMEDOUT);
    CHECK(ms_since(t0) >= 100.0 && b2.broken());
}

// A group that fails after a peer pulled one of its messages: the failing rank's stream still waits for
// that pull (its buffers may be reused in stream order). Rank 2 never comes; rank 1 only receives from
// rank 0 and succeeds. `first`: the position of the operation with the absent rank in rank 0's group;
// `recv_absent`: rank 0 fails in step 2 (a receive from rank 2), else in step 3 (a send to it).
static void failed_group_waits_for_pulls(bool recv_absent, bool first) {
    LocalBoard board(3);
    uint8_t src[8] = {1, 2, 3, 4, 5, 6, 7, 8}, dst[8] = {0}, other[8] = {0};
    FakeDev dev0, dev1;
    int rc1 = 1;
    std::thread t1([&] {
        std::vector<BoardOp> ops{BoardOp{false, 0, 0, dst, 8}};
        rc1 = board.run_group(1, ops, nullptr, 0, dev1, 60000);
    });
    const BoardOp to1{true, 1, 0, src, 8}, absent{!recv_absent, 2, 1, other, 8};
    std::vector<BoardOp> ops0 = first ? std::vector<BoardOp>{absent, to1} : std::vector<BoardOp>{to1, absent};
    CHECK(board.run_group(0, ops0, nullptr, 0, dev0, 300) == -ETIMEDOUT);
    t1.join();
    CHECK(rc1 == 0 && dev1.pulls == 1 && memcmp(src, dst, 8) == 0);
    CHECK(dev0.waits == 1 && dev0.pulls == 0 && board.broken());   // the one wait: rank 1's `pulled`
}

static void rank_slots() {
    LocalBoard board(2);
    CHECK(board.take_rank(2, 0) == -EINVAL && board.take_rank(-1, 0) == -EINVAL);
    CHECK(board.take_rank(1, 3) == 0 && board.take_rank(1, 0) == -EBUSY);
    CHECK(board.open_ranks() == 1 && board.device_of(1) == 3 && board.device_of(0) == -1);
    board.release_rank(1);
    CHECK(board.open_ranks() == 0 && board.take_rank(1, 0) == 0);
}

int main() {
    rank_slots();
    idle_rank();
    for (int world : {2, 3, 8}) all_pairs(world, 200);
    size_mismatch();
    absent_peer();
    for (int c = 0; c < 4; ++c) failed_group_waits_for_pulls((c & 1) != 0, (c & 2) != 0);
    printf("ok\n");
    return 0;
}
