/*
 * sr_slots.h — a framed offset back to its place in a slot arena (host only; C and C++).
 *
 * Datagrams that stay in their recvmmsg slots are framed on the device (sr_frame_slots, sr_route.h), so
 * the records' offsets refer to a framed stream the host never holds. ends[j] is the framed end offset
 * (exclusive) after datagram j (sr_frame_slots_size); an empty datagram repeats the previous value. A
 * datagram whose missing '\n' was written into its slot (there is room: a kept datagram is at most 4095
 * bytes of a 4096-byte slot) IS its framed form there, and a line never crosses a datagram, so a framed
 * line is one run of bytes in one slot.
 */
#ifndef SR_SLOTS_H
#define SR_SLOTS_H

#include <stddef.h>
#include <stdint.h>

/* The datagram that holds framed offset `off` (off < ends[count - 1]): the first j with ends[j] > off.
 * Never an empty datagram. */
static inline size_t sr_slot_of(const uint32_t *ends, size_t count, uint32_t off) {
    size_t lo = 0, hi = count;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (ends[mid] > off) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

/* Where framed byte `off` lies in an arena of slots `stride` bytes apart. */
static inline const uint8_t *sr_slot_addr(const uint8_t *arena, size_t stride, const uint32_t *ends, size_t count,
                                          uint32_t off) {
    const size_t j = sr_slot_of(ends, count, off);
    return arena + j * stride + (off - (j ? ends[j - 1] : 0u));
}

#endif /* SR_SLOTS_H */
