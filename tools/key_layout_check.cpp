// key_layout_check.cpp -- the container parser of a serialized ProvingKey (csrc/keyfmt.hpp) under AddressSanitizer / UBSan, on its own:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I mpc-jellyfish_amd/csrc tools/key_layout_check.cpp
//   ./a.out IMAGE CURVE_ID FLAGS
// IMAGE is a well-formed image (tests/test_key_io.py writes them).  Every parse runs on a heap copy of EXACTLY the bytes it is given, so
// that a read past [bytes, bytes + len) is a heap-buffer-overflow report.  It replays every truncation (each must be refused as
// "truncated") and sets every byte of every length prefix and tag to 0, 1, 2, 3 and 0xFF (each parse must end, accepted or refused).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "keyfmt.hpp"

using namespace mzk;

static bool parse_exact(const std::vector<uint8_t>& img, size_t len, int curve, uint32_t flags, mzk_key_layout_t* out, std::string* err) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(copy.get(), img.data(), len);
    keyfmt::Walk w(len ? copy.get() : nullptr, len);
    const bool ok = keyfmt::walk(w, curve, flags, out);
    *err = w.err;
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s IMAGE CURVE_ID FLAGS\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> img((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int curve = std::atoi(argv[2]);
    const uint32_t flags = (uint32_t)std::atoi(argv[3]);
    mzk_key_layout_t L, scratch;
    std::string err;
    if (!parse_exact(img, img.size(), curve, flags, &L, &err) || L.total_len != img.size()) { std::printf("the image itself is refused: %s\n", err.c_str()); return 1; }

    size_t truncations = 0;
    for (size_t len = 0; len < img.size(); len++, truncations++)
        if (parse_exact(img, len, curve, flags, &scratch, &err) || err.rfind("truncated in ", 0) != 0) {
            std::printf("prefix of %zu bytes: %s\n", len, err.empty() ? "accepted" : err.c_str());
            return 1;
        }

    // the bytes of every length prefix and tag
    std::vector<size_t> at;
    auto span = [&](uint64_t first, int n) { for (int i = 0; i < n; i++) at.push_back((size_t)first + i); };
    const uint64_t g2 = L.g2_record_bytes;
    if (!(flags & MZK_KEY_VK_ONLY)) {
        span(0, 8);
        for (uint32_t i = 0; i < L.num_wire_types; i++) span(L.sigma_off[i] - 8, 8);
        span(L.selector_off[0] - 16, 8);
        for (uint32_t i = 0; i < L.num_selectors; i++) span(L.selector_off[i] - 8, 8);
        span(L.commit_key_off - 8, 8);
        span(L.vk_off + L.vk_len, 1);
        for (int i = 0; L.has_plookup && i < 4; i++) span(L.table_off[i] - 8, 8);
    }
    span(L.vk_off, 16);
    span(L.sigma_comms_off - 8, 8);
    span(L.selector_comms_off - 8, 8);
    span(L.k_off - 8, 8);
    span(L.beta_h_off + g2, 2);
    size_t flips = 0, accepted = 0;
    static const uint8_t VALUES[5] = {0, 1, 2, 3, 0xFF};
    for (size_t pos : at)
        for (uint8_t v : VALUES) {
            const uint8_t keep = img[pos];
            img[pos] = v;
            accepted += parse_exact(img, img.size(), curve, flags, &scratch, &err) ? 1 : 0;
            img[pos] = keep;
            flips++;
        }
    std::printf("%zu truncations refused, %zu prefix / tag bytes x 5 values parsed (%zu accepted)\nok\n", truncations, at.size(), accepted);
    return 0;
}
