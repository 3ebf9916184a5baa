// Stand-alone check of the lock-step emulation of kp_introselect_block (kp_block_lockstep.h) against the scalar selection
// sm::kp_introselect_cp, meant to be built with -fsanitize=address,undefined (tests/test_kp_select_cpu.py does): the key
// buffers carry exactly the documented slack of four floats on either side and the stopper lists exactly num + 2 slots,
// so any scan that reads further, in either implementation, stops the program.
//   kp_block_lockstep_check exhaustive      every sequence over {0, 1, 2} of length 6 .. 11, every kth in 3 .. num - 2,
//                                           the switch to the parallel pass lowered to ranges of 6, both Pos flavours
//   kp_block_lockstep_check cases <file>    <file>: int32 count, then per case int32 num, int32 kth, float32 keys[num];
//                                           the real switch (256), both flavours
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kp_block_lockstep.h"

static int check_both(const float* v, int num, int kth, int par_min, const char* what, long id) {
    const int a = kp_lockstep::run_and_compare<unsigned short>(v, num, kth, par_min, nullptr, nullptr);
    const int b = kp_lockstep::run_and_compare<int>(v, num, kth, par_min, nullptr, nullptr);
    if (a || b) {
        printf("MISMATCH %s %ld: num %d kth %d (packed scan %d, int scans %d)\n", what, id, num, kth, a, b);
        if (num <= 16) {
            for (int i = 0; i < num; i++) printf(" %g", v[i]);
            printf("\n");
        }
    }
    return a | b;
}

static int exhaustive() {
    long runs = 0;
    int bad = 0;
    float v[11];
    for (int num = 6; num <= 11; num++) {
        long total = 1;
        for (int i = 0; i < num; i++) total *= 3;
        for (long code = 0; code < total; code++) {
            long c = code;
            for (int i = 0; i < num; i++) {
                v[i] = (float)(c % 3);
                c /= 3;
            }
            for (int kth = 3; kth <= num - 2; kth++) {
                bad |= check_both(v, num, kth, 6, "sequence", code);
                runs++;
            }
        }
    }
    printf("exhaustive: %ld selections\n", runs);
    return bad;
}

static int cases(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        printf("cannot open %s\n", path);
        return 2;
    }
    int n = 0, bad = 0;
    if (fread(&n, 4, 1, f) != 1) n = -1;
    for (int c = 0; c < n; c++) {
        int hdr[2];
        if (fread(hdr, 4, 2, f) != 2 || hdr[0] <= 0 || hdr[0] >= 65536 || hdr[1] < 0 || hdr[1] >= hdr[0]) {
            printf("bad case header %d\n", c);
            fclose(f);
            return 2;
        }
        std::vector<float> v(hdr[0]);
        if (fread(v.data(), 4, v.size(), f) != v.size()) {
            printf("short case %d\n", c);
            fclose(f);
            return 2;
        }
        bad |= check_both(v.data(), hdr[0], hdr[1], 256, "case", c);
    }
    fclose(f);
    printf("cases: %d selections\n", n);
    return n > 0 ? bad : 2;
}

int main(int argc, char** argv) {
    int rc = 2;
    if (argc == 2 && !strcmp(argv[1], "exhaustive")) rc = exhaustive();
    else if (argc == 3 && !strcmp(argv[1], "cases")) rc = cases(argv[2]);
    else printf("usage: %s exhaustive | cases <file>\n", argv[0]);
    if (rc == 0) printf("%s: ok\n", argv[1]);
    return rc;
}
