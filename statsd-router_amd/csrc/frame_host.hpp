// frame_host.hpp — framing arithmetic on the host (no HIP, no libc beyond the fixed-width types), so that
// a stand-alone program can include it (tools/frame_host_check.cpp).
//
// udp_read_cb keeps at most 4095 bytes of a datagram and appends '\n' unless the last kept byte is one
// (sr-main.c:163-173). A caller that leaves its datagrams in their recvmmsg slots and frames them on the
// device (sr_frame_slots) still needs the framed size on the host, for the route launch's grid: it is one
// byte looked at per datagram, none moved.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace srk {

constexpr uint32_t kFrameMaxDatagram = 4095;   // SR_MAX_DATAGRAM

// framed length of one datagram of `len` received bytes at `src` (0 for an empty one)
inline uint32_t frame_len(const uint8_t *src, size_t len) {
    const uint32_t n = len < kFrameMaxDatagram ? (uint32_t)len : kFrameMaxDatagram;
    if (n == 0) return 0;
    return n + (src[n - 1] != '\n' ? 1u : 0u);
}

// The framed total of `count` slots `stride` bytes apart; ends[j] (ends may be null) = the framed end
// offset (exclusive) after datagram j, so an empty datagram repeats the previous value.
inline size_t frame_slots_size(const uint8_t *slots, size_t stride, const uint16_t *lens, size_t count,
                               uint32_t *ends) {
    size_t pos = 0;
    for (size_t j = 0; j < count; ++j) {
        pos += frame_len(slots + j * stride, lens[j]);
        if (ends) ends[j] = (uint32_t)pos;
    }
    return pos;
}

}  // namespace srk
