// nexg_fixup.hip — nexg_recompute_checksums_batch: in-place checksum fix-up
// with the raw-buffer semantics of nex-packet's mutable views, chained as
// examples/mutable_chaining.rs:19-63 chains them (include/nexg.h):
//   MutableIpv4Packet::recompute_checksum  ipv4.rs:669-679  (header, skipword 5)
//   MutableUdpPacket::recompute_checksum   udp.rs:338-369   (pseudo, skipword 3)
//   MutableTcpPacket::recompute_checksum   tcp.rs:1009-1040 (pseudo, skipword 8)
//   MutableIcmpPacket::recompute_checksum  icmp.rs:372-377  (skipword 1)
//   MutableIcmpv6Packet::recompute_checksum icmpv6.rs:450-470 (pseudo, skipword 1)
// The checksums are util.rs:65-137 over each view's whole buffer (for the L4
// views: the enclosing IP view's payload_mut slice), in the same congruent
// closed form as the parse path (frame_core.hpp header): no re-serialisation.
//
// Not a streaming hot path (one lane per frame, 16-B loads through the frame,
// two 2-B byte-pair stores); the egress half of the checksum story.
#include "parse_kernels.hpp"

namespace nexg {

__global__ __launch_bounds__(256) void k_recompute(ParseArgs a, uint32_t which, nexg_fixup* out) {
    const uint64_t idx = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (idx >= a.count) return;
    nexg_fixup fx{0, 0, 0, 0, 0};
    uint64_t off;
    uint32_t len;
    if (!frame_extent(a, idx, off, len)) {
        if (out) out[idx] = fx;
        return;
    }
    fx = recompute_frame(const_cast<uint8_t*>(a.data) + off, len, a.opt_flags, a.ip_offset, which);
    if (out) out[idx] = fx;
}

hipError_t launch_recompute(const ParseArgs& a, uint32_t which, nexg_fixup* out, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const uint64_t blocks = (a.count + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_recompute, dim3((uint32_t)blocks), dim3(kTile), 0, s, a, which, out);
    return hipGetLastError();
}

}  // namespace nexg
