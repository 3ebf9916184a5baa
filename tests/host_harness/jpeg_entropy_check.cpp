// Stand-alone check of the host JPEG entropy pass (df-vo_amd/csrc/jpeg_entropy.h) on hostile input: no HIP, nothing but the
// header.  Built with -fsanitize=address,undefined and run by tests/test_jpeg_cpu.py:
//     jpeg_entropy_check <file.jpg> ...
// For every file: the file itself decodes; every strict prefix of it is refused; a few thousand seeded single-byte and
// double-byte corruptions each return DFVO_OK or DFVO_ERR_JPEG with a reason.  The input of every call is a heap block of
// exactly its length and the destination a heap block of exactly capacity + guard bytes, so a read or write outside either is
// the sanitizer's; the guard bytes behind the declared capacity keep their pattern.  Exit status 0 = every check holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../df-vo_amd/csrc/jpeg_entropy.h"

namespace {

enum { GUARD = 64, CORRUPTIONS = 3000 };

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

int failures = 0;

void expect(bool ok, const char* what, const char* file, long detail) {
    if (!ok) {
        fprintf(stderr, "%s: %s (%ld)\n", file, what, detail);
        failures++;
    }
}

// one call on an exact-size copy of the input into an exact-size destination; the return code
int call(const uint8_t* data, size_t n, size_t capacity, dfvo_jpeg_info* info, const char** reason, const char* file) {
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(in, data, n);
    uint8_t* dst = (uint8_t*)malloc(capacity + GUARD);
    memset(dst, 0xA5, capacity + GUARD);
    *reason = nullptr;
    const int rc = dfvo::jpeg::entropy_decode(n ? in : nullptr, n, dst, capacity, info, reason);
    for (int i = 0; i < GUARD; i++) expect(dst[capacity + i] == 0xA5, "guard byte overwritten", file, (long)i);
    expect(rc == DFVO_OK || (rc == DFVO_ERR_JPEG && *reason && **reason), "a return code that is neither OK nor a refusal with a reason", file,
           (long)rc);
    dfvo_jpeg_info probed;
    const char* why = nullptr;
    const int prc = dfvo::jpeg::probe(n ? in : nullptr, n, &probed, &why);
    expect(prc == DFVO_OK || prc == DFVO_ERR_JPEG, "probe: return code", file, (long)prc);
    if (rc == DFVO_OK) expect(prc == DFVO_OK && probed.bytes == info->bytes && info->bytes <= capacity, "probe and decode disagree", file, 0);
    free(dst);
    free(in);
    return rc;
}

void check_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        expect(false, "cannot open", path, 0);
        return;
    }
    std::vector<uint8_t> d;
    uint8_t chunk[4096];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) d.insert(d.end(), chunk, chunk + got);
    fclose(f);
    dfvo_jpeg_info info, scratch;
    const char* why;
    if (dfvo::jpeg::probe(d.data(), d.size(), &info, &why) != DFVO_OK) {
        expect(false, "probe refuses the file", path, 0);
        return;
    }
    const size_t cap = (size_t)info.bytes;
    expect(call(d.data(), d.size(), cap, &scratch, &why, path) == DFVO_OK, "the file itself is refused", path, 0);
    const int small = call(d.data(), d.size(), cap - 1, &scratch, &why, path);
    expect(small == DFVO_ERR_JPEG && why && strstr(why, "capacity"), "a capacity one byte too small is not refused by name", path, small);
    for (size_t n = 0; n < d.size(); n++)
        expect(call(d.data(), n, cap, &scratch, &why, path) == DFVO_ERR_JPEG, "a strict prefix decodes", path, (long)n);
    Rng rng{0x9E3779B97F4A7C15ull ^ d.size()};
    std::vector<uint8_t> m;
    long ok = 0;
    for (int i = 0; i < CORRUPTIONS; i++) {
        m = d;
        m[rng.next() % m.size()] = (uint8_t)rng.next();
        if (i & 1) m[rng.next() % m.size()] ^= (uint8_t)(1u << (rng.next() & 7));
        ok += call(m.data(), m.size(), cap, &scratch, &why, path) == DFVO_OK;
    }
    printf("%s: %zu bytes, %zu prefixes refused, %d corruptions (%ld still decode)\n", path, d.size(), d.size(), (int)CORRUPTIONS, ok);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: jpeg_entropy_check <file.jpg> ...\n");
        return 2;
    }
    for (int i = 1; i < argc; i++) check_file(argv[i]);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("jpeg_entropy_check: ok\n");
    return 0;
}
