// Stand-alone host check of the sizing / limit logic of maskunet_amd/csrc/rle.hip: every call returns before a launch, so it needs no
// GPU.  Meant for the host sanitizers (from the repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         maskunet_amd/csrc/rle.hip tools/rle_host_limits.cpp -o /tmp/rle_host_limits && /tmp/rle_host_limits
#include <cstdio>
#include <cstdlib>
#include "../include/maskunet_hip.h"
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
    CHECK(mu_rle_encode_supported(256, 256, 4096, 65536) == 0);
    CHECK(mu_rle_encode_supported(256, 257, 1, 1) == -2);
    CHECK(mu_rle_encode_supported(2147483647, 2147483647, 1, 1) == -2);
    CHECK(mu_rle_encode_supported(65536, 65537, 1, 1) == -2);
    CHECK(mu_rle_encode_supported(0, 1, 1, 1) == -2 && mu_rle_encode_supported(1, -1, 1, 1) == -2);
    CHECK(mu_rle_encode_supported(1, 1, 0, 1) == -2 && mu_rle_encode_supported(1, 1, 4097, 1) == -2);
    CHECK(mu_rle_encode_supported(1, 1, 1, 0) == -2 && mu_rle_encode_supported(1, 1, 1, 65537) == -2);
    CHECK(mu_rle_encode_supported(1, 1, 1, 1) == 0);
    // ints per image: table max_id + 1, boundaries 2 N, 16-bit rowmap (N + 1) / 2
    CHECK(mu_rle_encode_workspace_bytes(1, 1, 1, 1, 1) == (2 + 2 + 1) * 4);
    CHECK(mu_rle_encode_workspace_bytes(3, 5, 7, 9, 11) == 3L * (12 + 70 + 18) * 4);
    CHECK(mu_rle_encode_workspace_bytes(2147483647, 256, 256, 4096, 65536) == 2147483647L * (65537 + 131072 + 32768) * 4);
    CHECK(mu_rle_encode_workspace_bytes(0, 4, 4, 1, 1) == 0 && mu_rle_encode_workspace_bytes(-1, 4, 4, 1, 1) == 0);
    CHECK(mu_rle_encode_workspace_bytes(1, 256, 257, 1, 1) == 0);
    CHECK(mu_rle_decode_supported(256, 256, 4096) == 0 && mu_rle_decode_supported(256, 257, 1) == -2);
    CHECK(mu_rle_decode_supported(4, 4, 0) == -2 && mu_rle_decode_supported(4, 4, 4097) == -2 && mu_rle_decode_supported(-4, 4, 1) == -2);
    int buf[64];
    unsigned char* sb = (unsigned char*)buf;
    CHECK(mu_rle_encode(nullptr, buf, 1, 4, 4, 1, 1, buf, buf, buf, buf, sb, buf, 1 << 20, nullptr) == -1);
    CHECK(mu_rle_encode(buf, buf, 0, 4, 4, 1, 1, buf, buf, buf, buf, sb, buf, 1 << 20, nullptr) == -1);
    CHECK(mu_rle_encode(buf, buf, 1, 4, 4, 1, 1, buf, buf, buf, buf, sb + 1, buf, 1 << 20, nullptr) == -1);
    CHECK(mu_rle_encode(buf, buf, 1, 256, 257, 1, 1, buf, buf, buf, buf, sb, buf, 1L << 40, nullptr) == -2);
    CHECK(mu_rle_encode(buf, buf, 1, 4, 4, 4097, 1, buf, buf, buf, buf, sb, buf, 1L << 40, nullptr) == -2);
    CHECK(mu_rle_encode(buf, buf, 1, 4, 4, 1, 16, buf, buf, buf, buf, sb, buf, mu_rle_encode_workspace_bytes(1, 4, 4, 1, 16) - 1, nullptr) == -4);
    CHECK(mu_rle_decode(nullptr, buf, 1, 4, 4, 1, 64, buf, buf, nullptr) == -1);
    CHECK(mu_rle_decode(buf, buf, 1, 4, 4, 1, 0, buf, buf, nullptr) == -1);
    CHECK(mu_rle_decode(buf, buf, 1, 4, 4, 1, 1L << 31, buf, buf, nullptr) == -1);
    CHECK(mu_rle_decode(buf, buf, 1, 256, 257, 1, 64, buf, buf, nullptr) == -2);
    CHECK(mu_rle_decode(buf, buf, 1, 4, 4, 4097, 64, buf, buf, nullptr) == -2);
    printf("rle host logic OK\n");
    return 0;
}
