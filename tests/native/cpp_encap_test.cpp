// TEST INFRASTRUCTURE ONLY: the C++ host API's tunnel encapsulation
// (include/nexg.hpp nexg::Tunnel, nexg::TunnelSet, Engine::encap_plan / encap /
// encap_bufs) on the frames tests/test_cpp_encap.py writes, one hex frame per
// line ("-" = empty frame).
//   --link: no device; the wrappers are instantiated and linked, the struct
//           sizes and the builders' validation are checked
//   --gpu <file>: the four tunnels below with align 1, then 16, frame i under
//           tunnel i % 6 (4: past the set, 5: NEXG_TUNNEL_NONE): "W <align>
//           <frames> <total>", per frame "F <offset> <hex> <status> <tunnel>
//           <hdr_len> <src_port> <l4_csum>"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "nexg.hpp"

static std::vector<uint8_t> hex(const std::string& s) {
    std::vector<uint8_t> b;
    if (s == "-") return b;
    for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return b;
}

static const uint8_t kM1[6] = {0x02, 0xa0, 0xb0, 0xc0, 0xd0, 0xe1}, kM2[6] = {0x02, 0xa0, 0xb0, 0xc0, 0xd0, 0xe2};
static const uint8_t kS4[4] = {192, 0, 2, 1}, kD4[4] = {198, 51, 100, 7};
static const uint8_t kS6[16] = {0x20, 0x01, 0x0d, 0xb8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
static const uint8_t kD6[16] = {0x20, 0x01, 0x0d, 0xb8, 0, 0, 0, 0xff, 0, 0, 0xff, 0xff, 0, 0, 0, 7};  // 2001:db8:0:ff::ffff:0:7

// tests/test_cpp_encap.py builds the same four tunnels
static nexg::TunnelSet tunnels() {
    nexg::TunnelSet s;
    s.add(nexg::Tunnel::vxlan(4, kS4, kD4, 5001).macs(kM1, kM2).ports(49152, 0, 16384).udp_csum().ip(64, 0xB8, 0x1234, 2));
    s.add(nexg::Tunnel::vxlan(6, kS6, kD6, 0xABCDEF).macs(kM1, kM2).ports(40000, 8472).ip(33, 0x28, 0, 0, 0xABCDE));
    s.add(nexg::Tunnel::gre(4, kS4, kD4).macs(kM1, kM2).key(0xA1B2C3D4).sequence(0xFFFFFFF0).ip(255));
    s.add(nexg::Tunnel::gre(6, kS6, kD6).macs(kM1, kM2).l3().ip(1, 0, 0, 0, 7));
    return s;
}

static int run_gpu(const char* path) {
    std::vector<std::vector<uint8_t>> frames;
    std::ifstream in(path);
    for (std::string line; std::getline(in, line);)
        if (!line.empty()) frames.push_back(hex(line));
    std::vector<uint8_t> index(frames.size());
    for (size_t i = 0; i < index.size(); i++) index[i] = i % 6 == 5 ? NEXG_TUNNEL_NONE : (uint8_t)(i % 6);
    nexg::Engine eng(0);
    for (uint32_t align : {1u, 16u}) {
        const auto r = eng.encap_bufs(frames, tunnels(), index, align);
        printf("W %u %zu %llu\n", align, r.rows.size(), (unsigned long long)r.offsets.back());
        for (size_t i = 0; i < r.rows.size(); i++) {
            printf("F %llu ", (unsigned long long)r.offsets[i]);
            if (r.lengths[i] == 0) printf("-");
            for (uint32_t k = 0; k < r.lengths[i]; k++) printf("%02x", r.data[r.offsets[i] + k]);
            printf(" %u %u %u %u %u\n", r.rows[i].status, r.rows[i].tunnel, r.rows[i].hdr_len, r.rows[i].src_port, r.rows[i].l4_csum);
        }
    }
    return 0;
}

template <class F>
static int refuses(F f) {
    try {
        f();
    } catch (const nexg::Error&) {
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg_tunnel_spec) == 96 && sizeof(nexg_tunnels) == 8 + 16 * 96 && sizeof(nexg_encapped) == 8, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::encap_plan;
    auto p2 = &nexg::Engine::encap;
    auto p3 = &nexg::Engine::encap_bufs;
    int ok = 0, refused = 0;
    ok += nexg_tunnels_check(&tunnels().get()) == NEXG_OK;
    ok += tunnels().needs_flows();
    ok += !nexg::TunnelSet().add(nexg::Tunnel::gre(4, kS4, kD4)).needs_flows();
    const nexg::Tunnel good = nexg::Tunnel::vxlan(4, kS4, kD4, 1);
    refused += refuses([] { (void)nexg::TunnelSet().get(); });                                                // no tunnel
    refused += refuses([&] { nexg::TunnelSet s; for (int i = 0; i < 17; i++) s.add(good); });                // the 17th
    refused += refuses([] { (void)nexg::Tunnel::vxlan(5, kS4, kD4, 1); });                                    // family 5
    refused += refuses([] { (void)nexg::TunnelSet().add(nexg::Tunnel::vxlan(4, kS4, kD4, 1u << 24)).get(); });  // vni 2^24
    refused += refuses([&] { nexg::Tunnel t = good; t.key(1); (void)nexg::TunnelSet().add(t).get(); });       // a GRE flag on VXLAN
    refused += refuses([] { (void)nexg::TunnelSet().add(nexg::Tunnel::gre(4, kS4, kD4).udp_csum()).get(); });  // a VXLAN flag on GRE
    refused += refuses([&] { nexg::Tunnel t = good; t.t.flags = 0x20; (void)nexg::TunnelSet().add(t).get(); });  // unknown flag
    refused += refuses([&] { nexg::Tunnel t = good; t.ports(65535, 0, 2); (void)nexg::TunnelSet().add(t).get(); });  // past 65536
    refused += refuses([&] { nexg::Tunnel t = good; t.t.port_span = 1; (void)nexg::TunnelSet().add(t).get(); });  // span alone
    refused += refuses([&] { nexg::Tunnel t = good; t.ip(64, 0, 0, 8); (void)nexg::TunnelSet().add(t).get(); });  // ip_flags 8
    refused += refuses([&] { nexg::Tunnel t = good; t.ip(64, 0, 0, 0, 1u << 20); (void)nexg::TunnelSet().add(t).get(); });
    refused += refuses([&] { nexg::Tunnel t = good; t.t.reserved[22] = 1; (void)nexg::TunnelSet().add(t).get(); });
    refused += refuses([&] { nexg::TunnelSet s; s.add(good); s.s.reserved = 1; (void)s.get(); });
    printf("link ok %d %d %d\n", (p1 != nullptr) + (p2 != nullptr) + (p3 != nullptr), ok, refused);
    return 0;
}
