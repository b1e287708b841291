// Test infrastructure: a stand-alone program around the lockstep emulation of k_inflate (tests/inflate_emul.cpp), so that the
// decoder's source can run under AddressSanitizer and UndefinedBehaviorSanitizer as a program of its own (tests/test_inflate.py
// builds both files with -fsanitize=address,undefined and runs the result on the corpus of tests/deflate_craft.py).
//
// The corpus file (little-endian 32-bit words): the number of streams; per stream in_len, out_len, the class of the expected
// result (0: inflates to the text that follows, 1: an error, and nothing written outside the output), in_len bytes of raw DEFLATE
// stream, out_len bytes of expected text.  Every stream is decoded at three misalignments of the output, with the CRC-32 check and
// the list of line feeds on.  Exit status 0: everything as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" void pgi_emul_crc_setup(int on, uint32_t want);
extern "C" void pgi_emul_nl_setup(uint32_t cap, uint32_t lim);
extern "C" uint32_t pgi_emul_nl_result(uint16_t *out, uint32_t cap);
extern "C" int pgi_emul_inflate_at(const uint8_t *comp, uint32_t n_comp, uint32_t in_off, uint32_t in_len, uint8_t *dst, uint32_t out_len,
                                   int misalign);

static uint32_t crc32_of(const uint8_t *p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t k = 0; k < n; ++k) {
        c ^= p[k];
        for (int b = 0; b < 8; ++b) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
    }
    return ~c;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + n);
    fclose(f);
    size_t at = 0;
    auto word = [&](uint32_t *v) {
        if (at + 4 > file.size()) return false;
        std::memcpy(v, file.data() + at, 4);
        at += 4;
        return true;
    };
    uint32_t count = 0;
    if (!word(&count)) return 2;
    int bad = 0, runs = 0;
    for (uint32_t s = 0; s < count; ++s) {
        uint32_t in_len = 0, out_len = 0, cls = 0;
        if (!word(&in_len) || !word(&out_len) || !word(&cls) || at + (size_t)in_len + out_len > file.size()) return 2;
        const uint8_t *raw = file.data() + at, *text = raw + in_len;
        at += (size_t)in_len + out_len;
        std::vector<uint32_t> want_nl;
        for (uint32_t k = 0; k < out_len; ++k)
            if (text[k] == 10) want_nl.push_back(k);
        const int misalign[3] = {0, 7, 15};
        for (int m = 0; m < 3; ++m) {
            // the stream in a buffer of exactly its size plus what stands in front of it: a read behind it is the sanitizer's
            const uint32_t pre = (uint32_t)(s + 3u * (uint32_t)m) % 9u;
            std::vector<uint8_t> comp((size_t)pre + in_len, (uint8_t)0x5A);
            if (in_len) std::memcpy(comp.data() + pre, raw, in_len);
            std::vector<uint8_t> out((size_t)out_len + 1, (uint8_t)0xEE);
            std::vector<uint16_t> nl(70000);
            pgi_emul_crc_setup(1, crc32_of(text, out_len));
            pgi_emul_nl_setup(70000, 0xFFFFFFFFu);
            const int rc = pgi_emul_inflate_at(comp.data(), (uint32_t)comp.size(), pre, in_len, out.data(), out_len, misalign[m]);
            ++runs;
            bool ok;
            if (cls == 0) {
                ok = rc == 0 && std::memcmp(out.data(), text, out_len) == 0;
                const uint32_t n = pgi_emul_nl_result(nl.data(), 70000);
                ok = ok && n == want_nl.size();
                for (uint32_t k = 0; ok && k < n; ++k) ok = nl[k] == want_nl[k];
            } else {
                ok = rc != 0 && rc < (1 << 20);
            }
            if (!ok) {
                std::fprintf(stderr, "stream %u (class %u, %u -> %u bytes) at misalignment %d: rc %d\n", s, cls, in_len, out_len, misalign[m], rc);
                ++bad;
            }
        }
    }
    std::printf("%d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
