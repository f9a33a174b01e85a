// Stand-alone differential driver of the Deflate strip decoder (csrc/tiff_inflate.h) for tests/test_tiff_inflate.py: built
// with -fsanitize=address,undefined and linked with zlib, it walks a corpus of streams
//   corpus file: u32 count, then per case u32 raw (0: zlib stream, 1: raw Deflate) + u32 nout + u32 length + bytes (little endian)
// and decodes each one with zlib -- uncompress() for wrapped streams, inflateInit2(-15) for raw ones; accepted means the
// stream ends with exactly `nout` bytes out -- and with the shared text through both table arrangements, the host's words
// side by side and the kernel's strided ones.  The stream and every output lie in heap blocks of exactly their sizes, so one
// byte read or written beyond them is a sanitizer report.  The verdicts must be equal every time, and the bytes where the
// stream is accepted.  Prints one line of a letter per case, A accepted / R refused; any disagreement ends it with a failure.
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <memory>
#include <string>
#include <vector>

#include "tiff_inflate.h"

static bool get_u32(FILE* f, uint32_t* v) {
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
}

static bool zlib_accepts(const std::vector<uint8_t>& src, bool raw, std::vector<uint8_t>& out) {
    if (!raw) {
        uLongf got = (uLongf)out.size();
        return uncompress(out.data(), &got, src.data(), (uLong)src.size()) == Z_OK && got == out.size();
    }
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, -15) != Z_OK) return false;
    z.next_in = const_cast<Bytef*>(src.data());
    z.avail_in = (uInt)src.size();
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    int rc;
    do rc = inflate(&z, Z_NO_FLUSH); while (rc == Z_OK);  // (no progress possible: Z_BUF_ERROR)
    const bool ok = rc == Z_STREAM_END && z.total_out == out.size();
    inflateEnd(&z);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint32_t count = 0;
    if (!f || !get_u32(f, &count)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::unique_ptr<mrg::TiffInflateHostTable> host_table(new mrg::TiffInflateHostTable);
    constexpr uint32_t kStride = 3;
    std::string verdicts;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t raw = 0, nout = 0, len = 0;
        if (!get_u32(f, &raw) || !get_u32(f, &nout) || !get_u32(f, &len)) return 2;
        std::vector<uint8_t> src(len), ref(nout), a(nout), b(nout);
        if (len && fread(src.data(), 1, len, f) != len) return 2;
        const bool want = zlib_accepts(src, raw != 0, ref);
        // the strided words in a block of exactly their extent
        std::vector<uint16_t> words((size_t)(mrg::kTiffInflateWords - 1) * kStride + 1);
        mrg::TiffInflateStridedTable strided{words.data(), kStride};
        const int ra = raw ? mrg::tiff_inflate_raw(src.data(), len, a.data(), nout, *host_table)
                           : mrg::tiff_inflate_decode(src.data(), len, a.data(), nout, *host_table);
        const int rb = raw ? mrg::tiff_inflate_raw(src.data(), len, b.data(), nout, strided)
                           : mrg::tiff_inflate_decode(src.data(), len, b.data(), nout, strided);
        if (ra != rb) { fprintf(stderr, "case %u: the two table arrangements disagree: %d %d\n", i, ra, rb); return 3; }
        if ((ra == 0) != want) { fprintf(stderr, "case %u: zlib %s, the shared text returns %d\n", i, want ? "accepts" : "refuses", ra); return 3; }
        if (want && nout && (memcmp(ref.data(), a.data(), nout) || memcmp(ref.data(), b.data(), nout))) {
            fprintf(stderr, "case %u: accepted, other bytes than zlib's\n", i);
            return 3;
        }
        verdicts += want ? 'A' : 'R';
    }
    fclose(f);
    printf("%s\n", verdicts.c_str());
    return 0;
}
