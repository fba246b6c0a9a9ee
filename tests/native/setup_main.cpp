// setup_main.cpp -- the development setup's host path as a stand-alone program (tests/test_setup_host.py builds it with
// -fsanitize=address,undefined from setup_host.cpp and host_util.cpp only: no HIP code, no device).
//   setup_main <circuit.r1cs> <trapdoor.bin> <expected.zkey> <log_domain>
// trapdoor.bin: tau, alpha, beta, gamma, delta_round, delta_final as 32-byte little-endian integers. Makes the Groth16 key on
// host threads and exits 0 when it equals the expected file byte for byte, the size query agrees with what the run wrote, and a
// device run is refused (this program has none).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
#include "ultragroth_hip.h"

static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc != 5) { fputs("Usage: setup_main <circuit.r1cs> <trapdoor.bin> <expected.zkey> <log_domain>\n", stderr); return 2; }
    const std::vector<char> r1cs = slurp(argv[1]), td = slurp(argv[2]), want = slurp(argv[3]);
    if (td.size() != 192) { fputs("trapdoor.bin must hold six 32-byte values\n", stderr); return 2; }
    ug_setup_options opt;
    memset(&opt, 0, sizeof opt);
    opt.size = sizeof opt;
    opt.protocol = 1;
    opt.log_domain = (uint32_t)atoi(argv[4]);
    uint8_t* dst[6] = {opt.tau, opt.alpha, opt.beta, opt.gamma, opt.delta_round, opt.delta_final};
    for (int i = 0; i < 6; i++) memcpy(dst[i], td.data() + 32 * i, 32);
    char err[512] = "";
    uint64_t zbytes = 0, vmax = 0;
    if (ug_setup_size(&opt, r1cs.data(), r1cs.size(), &zbytes, &vmax, err, sizeof err) != UG_OK) { fprintf(stderr, "size: %s\n", err); return 1; }
    std::vector<char> zkey(zbytes), vkey(vmax);
    uint64_t wrote = 0, vlen = 0;
    if (ug_setup_run(&opt, r1cs.data(), r1cs.size(), -1, zkey.data(), zkey.size(), &wrote, vkey.data(), vkey.size(), &vlen, nullptr, err,
                     sizeof err) != UG_OK) {
        fprintf(stderr, "run: %s\n", err);
        return 1;
    }
    if (wrote != zbytes) { fprintf(stderr, "the run wrote %llu bytes, the size query said %llu\n", (unsigned long long)wrote, (unsigned long long)zbytes); return 1; }
    if (vlen + 1 > vmax || strlen(vkey.data()) != vlen) { fputs("verification key length\n", stderr); return 1; }
    if (zkey.size() != want.size() || memcmp(zkey.data(), want.data(), want.size()) != 0) {
        size_t at = 0;
        while (at < zkey.size() && at < want.size() && zkey[at] == want[at]) at++;
        fprintf(stderr, "the key differs from the expected file at byte %zu (%zu against %zu bytes)\n", at, zkey.size(), want.size());
        return 1;
    }
    if (ug_setup_run(&opt, r1cs.data(), r1cs.size(), 0, zkey.data(), zkey.size(), &wrote, vkey.data(), vkey.size(), &vlen, nullptr, err,
                     sizeof err) == UG_OK || strncmp(err, "setup: ", 7) != 0) {
        fputs("a device run was not refused\n", stderr);
        return 1;
    }
    puts("setup_main ok");
    return 0;
}
