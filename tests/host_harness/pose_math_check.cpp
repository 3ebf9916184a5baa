// Host build of df-vo_amd/csrc/pose_math.h (tests/test_pose_math_cpu.py): reads "<mult> p0 .. p5" lines from stdin, prints
// the 16 floats of pose_from_parameters for each as hexadecimal bit patterns.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../df-vo_amd/csrc/pose_math.h"

int main() {
    float mult, p[6];
    while (scanf("%f %f %f %f %f %f %f", &mult, &p[0], &p[1], &p[2], &p[3], &p[4], &p[5]) == 7) {
        float M[16];
        dfvo::pose_from_parameters(p, mult, M);
        for (int i = 0; i < 16; ++i) {
            uint32_t u;
            memcpy(&u, &M[i], 4);
            printf("%08x%c", u, i == 15 ? '\n' : ' ');
        }
    }
    return 0;
}
