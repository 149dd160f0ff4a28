// TEST INFRASTRUCTURE ONLY: the C++ host API's tunnel decapsulation
// (include/nexg.hpp Engine::decap / decap_select / decap_bufs) on the frames
// tests/test_cpp_decap.py writes, one hex frame per line ("-" = empty frame).
//   --link: no device; the wrappers are instantiated and linked, the header's
//           constants and struct sizes are checked
//   --gpu <file>: per frame "T <nexg_tunnel as 32 hex digits> <inner_off> <inner_len>",
//           then "S <mask> <count> <outer indices...>" for the Ethernet and IP classes
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

// a device-level pass with the thin wrappers: parse -> decap -> select
static int run_gpu(const char* path) {
    std::vector<std::vector<uint8_t>> frames;
    std::ifstream in(path);
    for (std::string line; std::getline(in, line);)
        if (!line.empty()) frames.push_back(hex(line));
    nexg::Engine eng(0);
    nexg::ParseOption vlan;
    vlan.unwrap_vlan = true;
    const auto d = eng.decap_bufs(frames, vlan);
    for (const auto& x : d) {
        const uint8_t* b = reinterpret_cast<const uint8_t*>(&x.tunnel);
        printf("T ");
        for (int i = 0; i < 16; i++) printf("%02x", b[i]);
        printf(" %u %u\n", x.inner_off, x.inner_len);
    }
    // select on the device from the same tunnels (uploaded again: decap_bufs owns its scratch)
    const uint64_t n = frames.size();
    std::vector<nexg_tunnel> tun(n);
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> len(n);
    for (uint64_t i = 0; i < n; i++) tun[i] = d[i].tunnel, off[i] = d[i].inner_off, len[i] = d[i].inner_len;
    nexg_tunnel* d_tun;
    uint64_t *d_off, *o_off;
    uint32_t *d_len, *o_idx, *o_len;
    const size_t m = n ? n : 1;
    if (hipMalloc(&d_tun, m * 16) || hipMalloc(&d_off, m * 8) || hipMalloc(&d_len, m * 4) || hipMalloc(&o_idx, m * 4) ||
        hipMalloc(&o_off, m * 8) || hipMalloc(&o_len, m * 4))
        return 2;
    if (hipMemcpy(d_tun, tun.data(), n * 16, hipMemcpyHostToDevice) || hipMemcpy(d_off, off.data(), n * 8, hipMemcpyHostToDevice) ||
        hipMemcpy(d_len, len.data(), n * 4, hipMemcpyHostToDevice))
        return 2;
    for (uint32_t mask : {1u << NEXG_INNER_ETHERNET, (1u << NEXG_INNER_IPV4) | (1u << NEXG_INNER_IPV6)}) {
        const uint64_t k = eng.decap_select(d_tun, d_off, d_len, n, mask, o_idx, o_off, o_len);
        std::vector<uint32_t> idx(k);
        if (k && hipMemcpy(idx.data(), o_idx, k * 4, hipMemcpyDeviceToHost)) return 2;
        printf("S %u %llu", mask, (unsigned long long)k);
        for (uint32_t i : idx) printf(" %u", i);
        printf("\n");
    }
    (void)hipFree(d_tun), (void)hipFree(d_off), (void)hipFree(d_len), (void)hipFree(o_idx), (void)hipFree(o_off), (void)hipFree(o_len);
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg_tunnel) == 16 && sizeof(nexg_decap_option) == 8, "include/nexg.h");
    static_assert(sizeof(nexg::Engine::Decap) == 24, "nexg_tunnel + two u32");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::decap;
    auto p2 = &nexg::Engine::decap_select;
    auto p3 = &nexg::Engine::decap_bufs;
    printf("link ok %d %llu %llu\n", (p1 != nullptr) + (p2 != nullptr) + (p3 != nullptr),
           (unsigned long long)nexg_decap_select_workspace(65793), (unsigned long long)nexg_decap_select_workspace(1));
    return 0;
}
