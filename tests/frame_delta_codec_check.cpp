// frame_delta_codec_check — the client's side of a packed delivery (csrc/zr_delta_codec.h, included alone: plain C++17, nothing of HIP)
// run over deliveries that tests/frame_delta_codec_reference.py encoded, under the sanitizers where the machine links them
// (tests/test_frame_delta_codec_cpu.py compiles and runs this; nothing of it is loaded into another process).
//
//   frame_delta_codec_check CASES.bin
// CASES.bin, little-endian 32-bit words: the number of cases, then per case  W H n bytes | tiles[n] | offsets[n + 1] | stream[bytes, padded
// to a whole word] | frame[W * H * 4].  Every buffer handed to the decoder is a heap block of exactly the size the call names, so that a
// read past tiles[n), offsets[n] or stream[bytes) is the sanitizer's to report.  Per case:
//   valid      the delivery applied to a copy filled with a sentinel: listed tiles equal the frame, everything else is still the sentinel
//   truncated  the same delivery with `bytes` cut short, at every 8-byte step of the last record and at a few odd lengths: refused, and
//              the copy is not touched
//   mutated    every byte of the header of the first, the last and the first raw record (8 bytes; a coded record's 32 width bytes as well)
//              set to every other value (pixel (0, 0), and frames above 64 x 64: every bit flipped alone): refused with the copy untouched, or - where the
//              changed record is still one the format allows - applied with nothing outside the listed tiles touched.  A changed
//              length word is always refused.
// One line per case; exit status 1 when anything failed.
#include "zr_delta_codec.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

static const uint8_t kSentinel = 0xA5;

template <typename T> static std::unique_ptr<T[]> exact(const T* src, size_t n)      // a heap block of exactly n elements (n == 0: one nobody may read)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    if (n) memcpy(p.get(), src, n * sizeof(T));
    return p;
}

struct Case {
    uint32_t W = 0, H = 0, n = 0, bytes = 0;
    std::vector<uint32_t> tiles, offsets;
    std::vector<uint8_t> stream, frame;
};

static bool read_words(FILE* f, uint32_t* dst, size_t n) { return fread(dst, 4, n, f) == n; }

static bool load(const char* path, std::vector<Case>& cases)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint32_t count = 0;
    bool ok = read_words(f, &count, 1) && count < 1000u;
    for (uint32_t k = 0; ok && k < count; ++k) {
        Case c;
        uint32_t head[4];
        ok = read_words(f, head, 4);
        if (!ok) break;
        c.W = head[0]; c.H = head[1]; c.n = head[2]; c.bytes = head[3];
        ok = c.W && c.H && c.W <= 4096u && c.H <= 4096u && c.n <= 65536u && c.bytes <= (64u << 20);
        if (!ok) break;
        c.tiles.resize(c.n); c.offsets.resize((size_t)c.n + 1u); c.stream.resize(((size_t)c.bytes + 3u) / 4u * 4u); c.frame.resize((size_t)c.W * c.H * 4u);
        ok = (!c.n || read_words(f, c.tiles.data(), c.n)) && read_words(f, c.offsets.data(), (size_t)c.n + 1u) &&
             (!c.bytes || fread(c.stream.data(), 1, c.stream.size(), f) == c.stream.size()) && fread(c.frame.data(), 1, c.frame.size(), f) == c.frame.size();
        cases.push_back(std::move(c));
    }
    fclose(f);
    return ok;
}

// listed[pixel]: the pixel lies in a tile the delivery lists
static std::vector<uint8_t> listed_pixels(const Case& c)
{
    std::vector<uint8_t> in((size_t)c.W * c.H, 0);
    const uint32_t tiles_x = (c.W + 31u) / 32u;
    for (uint32_t t : c.tiles)
        for (uint32_t y = t / tiles_x * 32u; y < c.H && y < t / tiles_x * 32u + 32u; ++y)
            for (uint32_t x = t % tiles_x * 32u; x < c.W && x < t % tiles_x * 32u + 32u; ++x) in[(size_t)y * c.W + x] = 1;
    return in;
}

static bool untouched(const std::vector<uint8_t>& client, const std::vector<uint8_t>& sentinel) { return memcmp(client.data(), sentinel.data(), client.size()) == 0; }

static bool outside_untouched(const std::vector<uint8_t>& client, const std::vector<uint8_t>& in)
{
    for (size_t p = 0; p < in.size(); ++p)
        if (!in[p] && (client[4 * p] != kSentinel || client[4 * p + 1] != kSentinel || client[4 * p + 2] != kSentinel || client[4 * p + 3] != kSentinel)) return false;
    return true;
}

int main(int argc, char** argv)
{
    std::vector<Case> cases;
    if (argc != 2 || !load(argv[1], cases)) { fprintf(stderr, "frame_delta_codec_check CASES.bin\n"); return 2; }
    int failed = 0;
    for (size_t k = 0; k < cases.size(); ++k) {
        const Case& c = cases[k];
        const std::vector<uint8_t> in = listed_pixels(c);
        const auto tiles = exact(c.tiles.data(), c.n);
        const auto offsets = exact(c.offsets.data(), (size_t)c.n + 1u);
        const auto stream = exact(c.stream.data(), c.bytes);
        const std::vector<uint8_t> sentinel(c.frame.size(), kSentinel);
        std::vector<uint8_t> client = sentinel;
        // valid
        bool valid = zr_codec_apply(tiles.get(), offsets.get(), c.n, stream.get(), c.bytes, c.W, c.H, client.data()) && outside_untouched(client, in);
        for (size_t p = 0; valid && p < in.size(); ++p)
            if (in[p] && memcmp(&client[4 * p], &c.frame[4 * p], 4) != 0) valid = false;
        // truncated
        uint32_t cuts = 0, cuts_refused = 0;
        if (c.n) {
            std::vector<uint32_t> at = { 0u, 1u, 7u, 8u, c.bytes - 1u, c.bytes - 7u };
            for (uint32_t b = c.offsets[c.n - 1u]; b < c.bytes; b += 8u) at.push_back(b);
            for (uint32_t cut : at) {
                if (cut >= c.bytes) continue;
                const auto part = exact(c.stream.data(), cut);
                client = sentinel;
                ++cuts;
                if (!zr_codec_apply(tiles.get(), offsets.get(), c.n, part.get(), cut, c.W, c.H, client.data()) && untouched(client, sentinel)) ++cuts_refused;
            }
        }
        // mutated
        client = sentinel;
        uint32_t mutated = 0, refused = 0, applied = 0, broken = 0, length = 0, length_refused = 0;
        const bool every_value = (size_t)c.W * c.H <= 64u * 64u;
        bool seen_raw = false;
        for (uint32_t r = 0; r < c.n; ++r) {
            uint8_t* rec = stream.get() + c.offsets[r];
            const bool raw = zr_codec_u16(rec + 6) == ZR_CODEC_RAW;
            if (r != 0u && r + 1u != c.n && (!raw || seen_raw)) continue;
            seen_raw = seen_raw || raw;
            for (uint32_t b = 0; b < (raw ? kZrCodecHeaderBytes : kZrCodecHeaderBytes + kZrCodecWidthBytes); ++b) {
                const uint8_t was = rec[b];
                for (uint32_t v = 0; v < 256u; ++v) {
                    if (v == was || ((!every_value || b < 4u) && ((v ^ was) & ((v ^ was) - 1u)))) continue;
                    rec[b] = (uint8_t)v;
                    const bool ok = zr_codec_apply(tiles.get(), offsets.get(), c.n, stream.get(), c.bytes, c.W, c.H, client.data());
                    ++mutated;
                    if (ok && outside_untouched(client, in)) ++applied;
                    else if (!ok && untouched(client, sentinel)) ++refused;
                    else ++broken;
                    if (ok) client = sentinel;
                    if (b == 4u || b == 5u) { ++length; length_refused += !ok; }
                }
                rec[b] = was;
            }
        }
        const bool good = valid && cuts_refused == cuts && broken == 0u && length_refused == length;
        printf("case %zu W=%u H=%u n=%u bytes=%u valid=%d truncated=%u truncated_refused=%u mutated=%u refused=%u applied=%u broken=%u length=%u length_refused=%u\n",
               k, c.W, c.H, c.n, c.bytes, (int)valid, cuts, cuts_refused, mutated, refused, applied, broken, length, length_refused);
        if (!good) failed = 1;
    }
    printf("cases %zu failed %d\n", cases.size(), failed);
    return failed;
}
