// Stand-alone check of sm::rigid_pose_inv_f32 (df-vo_amd/csrc/np_legacy.h), the closed-form rigid_flow_pose of the iterative
// scale loop's k_iter_begin, compiled for the host:  iter_pose_check <in> <out>
//   in:  int32 n, then n records of 17 float64 (E row-major 4x4, scale);  out: n records of 16 float32
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../df-vo_amd/csrc/np_legacy.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    if (fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 2;
    std::vector<double> in((size_t)n * 17);
    if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
    fclose(f);
    std::vector<float> out((size_t)n * 16);
    for (int i = 0; i < n; ++i) sm::rigid_pose_inv_f32(&in[(size_t)i * 17], in[(size_t)i * 17 + 16], &out[(size_t)i * 16]);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 2;
    fclose(f);
    printf("iter_pose: %d poses\n", (int)n);
    return 0;
}
