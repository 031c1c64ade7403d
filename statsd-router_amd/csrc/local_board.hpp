// local_board.hpp — the rendezvous board of the in-process communicator (include/sr_route.h:
// sr_comm_group_*, sr_comm_open_local). Plain C++17, no HIP types: events are opaque
// `void *` and the device work is three callbacks, so the whole protocol compiles and runs on the CPU
// (tools/local_board_check.cpp, also under ThreadSanitizer and AddressSanitizer).
//
// Ranks are threads of one process. A rank never copies to a peer: it POSTS {pointer, bytes, ready
// event} on the FIFO of the directed pair and tag, and the receiver PULLS (one device copy on its own
// stream, local_comm.hpp). One FIFO per (source, destination, tag): messages of one pair under one tag
// match in posting order.
//
// One group (run_group), on the calling rank's thread:
//   1. record one `ready` event on the own stream, then post every send of the group. Every rank posts
//      before it waits for anything, which is why no cycle of waiting ranks can form;
//   2. per posted receive, wait on the host (under the deadline) for the head message of the peer's
//      FIFO; sizes that differ give -EMSGSIZE and break the board. Then, in one critical section: the
//      own stream waits for each distinct ready event, ONE pull moves every segment of the group, one
//      `pulled` event is recorded and the messages are marked done with it;
//   3. per message this rank sent, wait on the host (under the deadline) until it is marked done; the
//      own stream then waits for the puller's event, so that the sender's later work on that stream
//      (the next launch's scatter into the packed buffer) is ordered after the pull, as after ncclSend.
// A rank waits only for the peers it has operations with; a group without operations returns at once.
//
// INVARIANT (the machines are shared): no device work is ever enqueued that waits on something not yet
// recorded. Every event is recorded before anyone is told about it, nothing on the device polls memory,
// and the `broken` flag is checked under the board's lock, which is still held while the pull is
// enqueued: a rank that gives up (deadline) breaks the board under the same lock, so a pull is either
// enqueued before its source's owner learns of the failure or not at all. A missing peer can therefore
// only cost host time, never a stuck stream.
//
// Failure: a deadline that runs out returns -ETIMEDOUT and breaks the board; a broken board wakes every
// waiter and every call on it from then on returns -EPIPE at once. A group that fails after it posted
// still orders the own stream after every pull of its messages that a peer enqueued before the board
// broke (there are no later ones), so send buffers may be reused in stream order after a failure too.
#pragma once

#include <errno.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

namespace srk {

constexpr int kBoardTags = 4;        // sr_transport's 0 (lines), 1 (records), 2 (dead rows); 3: the all-to-all
constexpr int kBoardA2ATag = 3;

struct BoardOp {   // one posted operation of a group
    bool is_send;
    int peer, tag;
    void *buf;
    size_t bytes;
};

struct BoardSeg {   // one copy of a pull
    const void *src;
    void *dst;
    size_t bytes;
};

// What run_group needs of the device (local_comm.hpp: HIP; the check program: fakes):
//   int record(void **ev)                      record an event on the own stream, *ev = its handle
//   int wait(void *ev)                         the own stream waits for a recorded event
//   int pull(const BoardSeg *segs, size_t n)   enqueue the copies on the own stream
// each returning 0 or a negative errno.

class LocalBoard {
  public:
    explicit LocalBoard(int world) : world_(world), fifos_((size_t)world * world * kBoardTags), device_(world, -1) {}

    int world() const { return world_; }

    // rank slots (sr_comm_open_local / sr_comm_close)
    int take_rank(int rank, int device) {
        std::lock_guard<std::mutex> lk(mu_);
        if (rank < 0 || rank >= world_) return -EINVAL;
        if (device_[rank] >= 0) return -EBUSY;
        device_[rank] = device;
        ++open_;
        return 0;
    }
    void release_rank(int rank) {
        std::lock_guard<std::mutex> lk(mu_);
        if (rank >= 0 && rank < world_ && device_[rank] >= 0) device_[rank] = -1, --open_;
    }
    int open_ranks() {
        std::lock_guard<std::mutex> lk(mu_);
        return open_;
    }
    int device_of(int rank) {   // -1: not open
        std::lock_guard<std::mutex> lk(mu_);
        return rank >= 0 && rank < world_ ? device_[rank] : -1;
    }

    bool broken() {
        std::lock_guard<std::mutex> lk(mu_);
        return broken_;
    }
    void break_all() {
        std::lock_guard<std::mutex> lk(mu_);
        break_locked();
    }

    // One group of `rank`: ops in posting order, plus copies within the rank itself (the own element of
    // an all-to-all) that ride in the same pull. timeout_ms 0: no deadline.
    template <class Dev>
    int run_group(int rank, const std::vector<BoardOp> &ops, const BoardSeg *local, size_t n_local, Dev &dev,
                  uint32_t timeout_ms) {
        if (rank < 0 || rank >= world_) return -EINVAL;
        size_t n_send = 0, n_recv = 0;
        for (const BoardOp &o : ops) {
            if (o.peer < 0 || o.peer >= world_ || o.peer == rank || o.tag < 0 || o.tag >= kBoardTags) return -EINVAL;
            (o.is_send ? n_send : n_recv)++;
        }
        if (broken()) return -EPIPE;
        if (!n_send && !n_recv && !n_local) return 0;
        const bool bounded = timeout_ms != 0;
        const Clock::time_point deadline = Clock::now() + std::chrono::milliseconds(timeout_ms);

        // 1. the ready event first, then the posts: nobody hears of an event that is not recorded
        struct Ticket {
            Fifo *f;
            uint64_t seq;
        };
        std::vector<Ticket> sent, taken;
        // A group that fails after its posts (lock held, board broken): peers that enqueued before the
        // board broke may have pulled some of this rank's messages. No pull is enqueued on a broken
        // board, so the `pulled` events visible now are all there will ever be: the own stream waits
        // for them, and the caller may reuse its send buffers in stream order as after a success.
        auto settle_locked = [&](int err) {
            std::vector<void *> evs;
            for (const Ticket &t : sent) {
                if (t.seq < t.f->base) continue;   // retired in step 3: already waited for
                const Msg &m = t.f->q[(size_t)(t.seq - t.f->base)];
                if (m.done && m.pulled) add_distinct(evs, m.pulled);
            }
            for (void *ev : evs) (void)dev.wait(ev);
            return err;
        };
        void *ready = nullptr;
        int rc = n_send ? dev.record(&ready) : 0;
        if (rc) return fail(rc);
        if (n_send) {
            std::unique_lock<std::mutex> lk(mu_);
            if (broken_) return -EPIPE;
            for (const BoardOp &o : ops) {
                if (!o.is_send) continue;
                Fifo &f = fifo(rank, o.peer, o.tag);
                sent.push_back({&f, f.base + f.q.size()});
                f.q.push_back(Msg{o.buf, o.bytes, ready, nullptr, false});
            }
            wake_locked();
        }

        // 2. the heads of the peers' FIFOs, then one pull for all of them
        std::vector<BoardSeg> segs(local, local + n_local);
        std::vector<void *> events;
        for (const BoardOp &o : ops) {
            if (o.is_send) continue;
            Fifo &f = fifo(o.peer, rank, o.tag);
            std::unique_lock<std::mutex> lk(mu_);
            rc = wait_locked(lk, bounded, deadline, [&] { return f.claimed < f.base + f.q.size(); });
            if (rc) return settle_locked(rc);
            const Msg &m = f.q[(size_t)(f.claimed - f.base)];
            if (m.bytes != o.bytes) {
                break_locked();
                return settle_locked(-EMSGSIZE);
            }
            taken.push_back({&f, f.claimed++});
            segs.push_back(BoardSeg{m.ptr, o.buf, o.bytes});
            add_distinct(events, m.ready);
        }
        if (!segs.empty()) {
            std::unique_lock<std::mutex> lk(mu_);
            if (broken_) return settle_locked(-EPIPE);
            for (void *ev : events)
                if ((rc = dev.wait(ev))) break;
            if (!rc) rc = dev.pull(segs.data(), segs.size());
            void *pulled = nullptr;
            if (!rc && !taken.empty()) rc = dev.record(&pulled);
            if (rc) {
                break_locked();
                return settle_locked(rc);
            }
            for (const Ticket &t : taken) {
                Msg &m = t.f->q[(size_t)(t.seq - t.f->base)];
                m.pulled = pulled;
                m.done = true;
            }
            if (!taken.empty()) wake_locked();
        }

        // 3. my messages pulled: the own stream is ordered after each puller
        events.clear();
        for (const Ticket &t : sent) {
            std::unique_lock<std::mutex> lk(mu_);
            rc = wait_locked(lk, bounded, deadline, [&] { return t.f->q[(size_t)(t.seq - t.f->base)].done; });
            if (rc) {
                for (void *ev : events) (void)dev.wait(ev);   // (of the messages retired so far)
                return settle_locked(rc);
            }
            add_distinct(events, t.f->q[(size_t)(t.seq - t.f->base)].pulled);
            // retire the messages that are done from the front (this rank is the FIFO's only sender)
            while (!t.f->q.empty() && t.f->q.front().done && t.f->base <= t.seq) t.f->q.pop_front(), ++t.f->base;
        }
        for (void *ev : events)
            if ((rc = dev.wait(ev))) return fail(rc);
        return 0;
    }

  private:
    using Clock = std::chrono::steady_clock;
    struct Msg {
        const void *ptr;
        size_t bytes;
        void *ready;    // recorded on the sender's stream before the post
        void *pulled;   // recorded on the receiver's stream after its pull, before `done`
        bool done;
    };
    struct Fifo {
        std::deque<Msg> q;      // messages base, base + 1, ...
        uint64_t base = 0;      // sequence number of q.front()
        uint64_t claimed = 0;   // the next message the receiver takes
    };

    Fifo &fifo(int src, int dst, int tag) { return fifos_[((size_t)src * world_ + dst) * kBoardTags + tag]; }

    static void add_distinct(std::vector<void *> &v, void *e) {
        for (void *x : v)
            if (x == e) return;
        v.push_back(e);
    }

    void wake_locked() {
        version_.fetch_add(1, std::memory_order_release);
        cv_.notify_all();
    }
    void break_locked() {
        broken_ = true;
        wake_locked();
    }
    int fail(int rc) {
        break_all();
        return rc;
    }

    static void relax() {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#else
        std::this_thread::yield();
#endif
    }

    // Wait (lock held on entry and on return) until pred() or the board breaks: a bounded spin on the
    // board's version word outside the lock, then the condition variable. -EPIPE: broken; -ETIMEDOUT: the
    // deadline ran out, and the board is broken by it.
    template <class Pred>
    int wait_locked(std::unique_lock<std::mutex> &lk, bool bounded, Clock::time_point deadline, Pred pred) {
        for (;;) {
            if (broken_) return -EPIPE;
            if (pred()) return 0;
            if (bounded && Clock::now() >= deadline) {
                break_locked();
                return -ETIMEDOUT;
            }
            const uint64_t v = version_.load(std::memory_order_acquire);
            lk.unlock();
            for (int i = 0; i < kSpin && version_.load(std::memory_order_acquire) == v; ++i) relax();
            lk.lock();
            if (version_.load(std::memory_order_acquire) != v) continue;   // something was posted or marked
            // (the wall clock only carries the wait; the deadline itself is re-read from the steady clock)
            if (bounded) cv_.wait_until(lk, std::chrono::system_clock::now() + (deadline - Clock::now()));
            else cv_.wait(lk);
        }
    }

    static constexpr int kSpin = 2000;
    const int world_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::atomic<uint64_t> version_{0};
    bool broken_ = false;
    int open_ = 0;
    std::vector<Fifo> fifos_;
    std::vector<int> device_;
};

}  // namespace srk
