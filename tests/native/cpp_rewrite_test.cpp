// TEST INFRASTRUCTURE ONLY: the C++ host API's header rewrite
// (include/nexg.hpp nexg::Action, nexg::ActionSet, Engine::rewrite /
// rewrite_bufs) on the frames tests/test_cpp_rewrite.py writes, one hex frame
// per line ("-" = empty frame).
//   --link: no device; the wrappers are instantiated and linked, the struct
//           sizes and the builders' validation are checked
//   --gpu <file>: the set below in RECOMPUTE, then in INCREMENTAL mode, frame i
//           under action i % 5 (3 and 4: past the set): "W <mode> <frames>", per
//           frame "F <hex> <applied> <fixed> <action> <ip_csum> <l4_csum>"
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
static const uint8_t kD6[16] = {0x20, 0x01, 0x0d, 0xb8, 0, 0xff, 0, 0, 0, 0, 0xff, 0xff, 0, 0, 0, 7};

// tests/test_cpp_rewrite.py builds the same three actions
static nexg::ActionSet actions(bool incremental) {
    nexg::ActionSet s;
    s.add(nexg::Action().nat4(kS4, kD4).ports(40000, 443).dec_ttl(1));
    s.add(nexg::Action().nat6(kS6, kD6).src_port(9).set_tos(0x28, 0xFC).mac(kM1, kM2));
    s.add(nexg::Action().set_ttl(7));
    return s.incremental(incremental);
}

static int run_gpu(const char* path) {
    std::vector<std::vector<uint8_t>> frames;
    std::ifstream in(path);
    for (std::string line; std::getline(in, line);)
        if (!line.empty()) frames.push_back(hex(line));
    std::vector<uint8_t> index(frames.size());
    for (size_t i = 0; i < index.size(); i++) index[i] = i % 5 == 4 ? NEXG_ACTION_NONE : (uint8_t)(i % 5);
    nexg::Engine eng(0);
    for (int mode = 0; mode < 2; mode++) {
        auto work = frames;
        const auto rows = eng.rewrite_bufs(work, actions(mode != 0), index);
        printf("W %d %zu\n", mode, rows.size());
        for (size_t i = 0; i < rows.size(); i++) {
            printf("F ");
            if (work[i].empty()) printf("-");
            for (uint8_t b : work[i]) printf("%02x", b);
            printf(" %u %u %u %u %u\n", rows[i].applied, rows[i].fixed, rows[i].action, rows[i].ip_csum, rows[i].l4_csum);
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
    static_assert(sizeof(nexg_action) == 64 && sizeof(nexg_actions) == 1032 && sizeof(nexg_rewritten) == 8, "include/nexg.h");
    if (argc >= 3 && std::string(argv[1]) == "--gpu") {
        try {
            return run_gpu(argv[2]);
        } catch (const std::exception& e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    // --link: take the wrappers' addresses so they are instantiated and must link
    auto p1 = &nexg::Engine::rewrite;
    auto p2 = &nexg::Engine::rewrite_bufs;
    int ok = 0, refused = 0;
    for (int mode = 0; mode < 2; mode++) ok += nexg_actions_check(&actions(mode != 0).get()) == NEXG_OK;
    ok += nexg_actions_check(&nexg::ActionSet().add(nexg::Action()).get()) == NEXG_OK;  // "leave it" is valid
    const nexg::Action good = nexg::Action().nat4(kS4, kD4);
    refused += refuses([] { (void)nexg::ActionSet().get(); });                                               // no action
    refused += refuses([&] { nexg::ActionSet s; for (int i = 0; i < 17; i++) s.add(good); });               // the 17th
    refused += refuses([&] { nexg::ActionSet s; s.add(good); s.s.flags = 0x2; (void)s.get(); });            // unknown flag
    refused += refuses([&] { nexg::Action a = good; a.a.sets |= 0x200; (void)nexg::ActionSet().add(a).get(); });  // unknown sets bit
    refused += refuses([&] { nexg::Action a = good; a.a.reserved[3] = 1; (void)nexg::ActionSet().add(a).get(); });
    refused += refuses([] { (void)nexg::ActionSet().add(nexg::Action().set_ttl(1).dec_ttl(1)).get(); });   // both TTL forms
    refused += refuses([] { (void)nexg::ActionSet().add(nexg::Action().dec_ttl(0)).get(); });
    refused += refuses([] { nexg::Action a; a.a.sets = NEXG_SET_IP_SRC; (void)nexg::ActionSet().add(a).get(); });  // family 0
    refused += refuses([] { nexg::Action a; a.ip_src(5, kS4); });
    refused += refuses([] { nexg::Action a; a.ip_src(4, kS4).ip_dst(6, kD6); });                            // two families
    refused += refuses([] { nexg::Action a; a.a.family = 4; (void)nexg::ActionSet().add(a).get(); });       // a family alone
    refused += refuses([] { (void)nexg::ActionSet().add(nexg::Action().set_tos(0, 0)).get(); });            // empty mask
    refused += refuses([] { (void)nexg::ActionSet().add(nexg::Action().set_tos(4, 3)).get(); });            // bits outside it
    printf("link ok %d %d %d\n", (p1 != nullptr) + (p2 != nullptr), ok, refused);
    return 0;
}
