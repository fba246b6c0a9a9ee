// main_zkey_new.cpp -- `zkey_new <circuit.r1cs> <prepared.ptau> <out.zkey> <out_vkey.json> [--delta draw|<file>] [--log-domain n]
//                                [--validate 0|1|2] [--device d]`
// A Groth16 proving key and its verification key from a circuit and a powers-of-tau file prepared for phase 2, on top of
// include/ultragroth_hip.h (ug_setup_ptau_*): what `snarkjs zkey new` does, then optionally ONE delta contribution.
//   --delta draw     a delta is drawn from OS entropy, applied and wiped; it is never written anywhere
//   --delta <file>   32 bytes, little-endian, below r, not 0
//   --device d       -1 runs on host threads (default: ULTRAGROTH_DEVICE, else 0)
// The .ptau is mapped, never read whole. No transcript is written: `snarkjs zkey verify` will not accept the key.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "cli_util.hpp"
#include "host_util.hpp"
#include "../../include/ultragroth_hip.h"

int main(int argc, char** argv) {
    const char* usage = "Usage: zkey_new <circuit.r1cs> <prepared.ptau> <out.zkey> <out_vkey.json> [--delta draw|<file>] [--log-domain n] [--validate 0|1|2] [--device d]\n";
    std::vector<std::string> pos;
    std::string delta;
    long logDomain = 0, validate = 1, device = ugcli::defaultDevice();
    const std::vector<ugcli::Option> options = {ugcli::textOption("--delta", &delta),
                                                ugcli::numberOption("--log-domain", &logDomain, 0, 64, "Error: --log-domain takes a number\n"),
                                                ugcli::validateOption(&validate, 0, "Error: --validate takes 0, 1 or 2\n"), ugcli::deviceOption(&device)};
    if (!ugcli::parseArgs(argc, argv, options, usage, pos)) return EXIT_FAILURE;
    if (pos.size() != 4) { fputs("Invalid number of parameters\n", stderr); fputs(usage, stderr); return EXIT_FAILURE; }
    try {
        ug_setup_ptau_options opt;
        memset(&opt, 0, sizeof opt);
        opt.size = sizeof opt;
        opt.log_domain = (uint32_t)logDomain;
        opt.validate = (uint32_t)validate;
        if (delta.empty()) {
            fputs("zkey_new: no contribution: delta = 1. ANYONE can forge proofs for this key until a contribution is applied.\n", stderr);
        } else if (delta == "draw") {
            opt.contribute = 2;
            fputs("zkey_new: a single-party phase 2 with no transcript: the key is sound only if this run's delta is gone and the .ptau is "
                  "honest, and `snarkjs zkey verify` will not accept it.\n", stderr);
        } else {
            opt.contribute = 1;
            ughost::FileMap d(delta);
            if (d.size() != 32) throw std::invalid_argument("--delta: the file must hold 32 bytes (little-endian, below r, not 0)");
            memcpy(opt.delta, d.data(), 32);
            fputs("zkey_new: a delta from a file: whoever can read that file forges proofs for this key.\n", stderr);
        }
        char message[1024] = {0};
        ughost::FileMap r1cs(pos[0]), ptau(pos[1]);
        uint64_t zbytes = 0, vmax = 0;
        if (ug_setup_ptau_size(&opt, r1cs.data(), r1cs.size(), ptau.data(), ptau.size(), &zbytes, &vmax, message, sizeof(message) - 1) != UG_OK)
            throw std::runtime_error(message);
        std::vector<uint8_t> zkey(zbytes);
        std::vector<char> vkey(vmax);
        double ms[UG_SETUP_PTAU_PHASES];
        uint64_t vlen = 0;
        const int rc = ug_setup_ptau_run(&opt, r1cs.data(), r1cs.size(), ptau.data(), ptau.size(), (int)device, zkey.data(), zkey.size(), &zbytes,
                                         vkey.data(), vkey.size(), &vlen, ms, message, sizeof(message) - 1);
        volatile uint8_t* w = opt.delta;
        for (int i = 0; i < 32; i++) w[i] = 0;
        if (rc != UG_OK) throw std::runtime_error(message);
        ugcli::writeFile(pos[2], zkey.data(), zbytes);
        ugcli::writeFile(pos[3], vkey.data(), vlen);
        printf("key written: %llu bytes (parse %.1f | point check %.1f | G1 combinations %.1f | G2 combination %.1f | delta %.1f | assembly %.1f ms)\n",
               (unsigned long long)zbytes, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
        return EXIT_SUCCESS;
    } catch (const std::exception& e) {
        fprintf(stderr, "Error: %s\n", e.what());
    }
    return EXIT_FAILURE;
}
