// TEST INFRASTRUCTURE ONLY: the C++ host API's DNS message pass
// (include/nexg.hpp Engine::dns / dns_entries / dns_bufs, nexg::decode_dns_name)
// on the frames tests/test_cpp_dns.py writes, one hex frame per line ("-" =
// empty frame).
//   --link: no device; the wrappers are instantiated and linked, the header's
//           struct sizes are checked and decode_dns_name runs on its vectors
//   --gpu <file>: per frame "D <nexg_dns as 64 hex digits> <first row>", then per
//           entry "E <nexg_dns_entry as 32 hex digits>" followed, for a query, by
//           its decoded name ("=name") or the error kind ("!Kind")
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

static void put_hex(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; i++) printf("%02x", b[i]);
}

static int run_gpu(const char* path) {
    std::vector<std::vector<uint8_t>> frames;
    std::ifstream in(path);
    for (std::string line; std::getline(in, line);)
        if (!line.empty()) frames.push_back(hex(line));
    nexg::Engine eng(0);
    nexg::ParseOption vlan;
    vlan.unwrap_vlan = true;
    const auto d = eng.dns_bufs(frames, vlan);
    for (size_t i = 0; i < frames.size(); i++) {
        printf("D ");
        put_hex(&d.dns[i], sizeof(nexg_dns));
        printf(" %llu\n", (unsigned long long)d.row[i]);
        const nexg_dns& s = d.dns[i];
        for (uint64_t k = d.row[i]; k < d.row[i + 1]; k++) {
            const nexg_dns_entry& e = d.entries[k];
            printf("E ");
            put_hex(&e, sizeof(e));
            if (e.section == 0) {
                // the qname bytes alone, as DnsQueryPacket::qname_parsed decodes them
                const uint8_t* q = frames[i].data() + s.msg_off + e.off;
                const auto r = nexg::decode_dns_name(q, e.name, 0);
                if (r.is_ok()) printf(" =%s", r.value().name.c_str());
                else printf(" !%s", r.error());
            }
            printf("\n");
        }
    }
    return 0;
}

static bool name_is(const std::vector<uint8_t>& b, size_t start, const char* want, size_t consumed) {
    const auto r = nexg::decode_dns_name(b.data(), b.size(), start);
    return r.is_ok() && r.value().name == want && r.value().consumed == consumed;
}

static bool name_fails(const std::vector<uint8_t>& b, const char* kind) {
    const auto r = nexg::decode_dns_name(b.data(), b.size(), 0);
    return r.is_err() && std::string(r.error()) == kind;
}

int main(int argc, char** argv) {
    static_assert(sizeof(nexg_dns) == 32 && sizeof(nexg_dns_entry) == 16 && sizeof(nexg_dns_option) == 8, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::dns;
    auto p2 = &nexg::Engine::dns_entries;
    auto p3 = &nexg::Engine::dns_bufs;
    // dns.rs:1499-1519 and the error kinds
    int ok = 0;
    ok += name_is(hex("03777777c006076578616d706c6503636f6d00"), 0, "www.example.com", 6);
    ok += name_is(hex("00"), 0, "", 1);
    ok += name_is(hex("ff0361626300"), 1, "abc", 5);
    ok += name_fails(hex("c000"), "CompressionLoop");
    ok += name_fails(hex("c002"), "InvalidCompression");
    ok += name_fails(hex("406100"), "InvalidCompression");
    ok += name_fails(hex("0361"), "Truncated");
    ok += name_fails(hex("02fffe00"), "InvalidUtf8");
    ok += name_fails(hex("03eda08000"), "InvalidUtf8");  // a surrogate
    ok += name_is(hex("03e2829c00"), 0, "\xe2\x82\x9c", 5);
    printf("link ok %d %d %llu %llu\n", (p1 != nullptr) + (p2 != nullptr) + (p3 != nullptr), ok,
           (unsigned long long)nexg_dns_tile_first_bytes(65537), (unsigned long long)nexg_dns_tile_first_bytes(0));
    return 0;
}
