// main_zkey_new.cpp -- `zkey_new <circuit.r1cs> <prepared.ptau> <out.zkey> <out_vkey.json> [--delta draw|<file>] [--log-domain n]
//                                [--validate 0|1|2] [--device d]`
// A Groth16 proving key and its verification key from a circuit and a powers-of-tau file prepared for phase 2, on top of
// include/ultragroth_hip.h (ug_setup_ptau_*): what `snarkjs zkey new` does, then optionally ONE delta contribution.
//   --delta draw     a delta is drawn from OS entropy, applied and wiped; it is never written anywhere
//   --delta <file>   32 bytes, little-endian, below r, not 0
//   --device d       -1 runs on host threads (default: ULTRAGROTH_DEVICE, else 0)
// The .ptau is mapped, never read whole. No transcript is written: `snarkjs zkey verify` will not accept the key.
//
// Built with -DUG_ULTRA: `zkey_new_ultra <circuit.r1cs> <prepared.ptau> <spec.json> <out.zkey> <out_vkey.json> [the same options]`,
// an UltraGroth (protocol 1337) key on top of ug_ultra_setup_ptau_*. spec.json is dev_setup --ultra's file: {"rand_indx",
// "round_signals", "final_signals"}. --delta draw draws BOTH deltas, independently; --delta <file> holds 64 bytes, delta_round then
// delta_final, each little-endian, below r, not 0.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "cli_util.hpp"
#include "host_util.hpp"
#include "../../include/ultragroth_hip.h"
#ifdef UG_ULTRA
#include "cli_spec.hpp"
#define TOOL "zkey_new_ultra"
#define POSITIONAL "<circuit.r1cs> <prepared.ptau> <spec.json> <out.zkey> <out_vkey.json>"
typedef ug_ultra_setup_ptau_options Options;
constexpr size_t N_POS = 5, DELTA_BYTES = 64;
#else
#define TOOL "zkey_new"
#define POSITIONAL "<circuit.r1cs> <prepared.ptau> <out.zkey> <out_vkey.json>"
typedef ug_setup_ptau_options Options;
constexpr size_t N_POS = 4, DELTA_BYTES = 32;
#endif

int main(int argc, char** argv) {
    const char* usage = "Usage: " TOOL " " POSITIONAL " [--delta draw|<file>] [--log-domain n] [--validate 0|1|2] [--device d]\n";
    std::vector<std::string> pos;
    std::string delta;
    long logDomain = 0, validate = 1, device = ugcli::defaultDevice();
    const std::vector<ugcli::Option> options = {ugcli::textOption("--delta", &delta),
                                                ugcli::numberOption("--log-domain", &logDomain, 0, 64, "Error: --log-domain takes a number\n"),
                                                ugcli::validateOption(&validate, 0, "Error: --validate takes 0, 1 or 2\n"), ugcli::deviceOption(&device)};
    if (!ugcli::parseArgs(argc, argv, options, usage, pos)) return EXIT_FAILURE;
    if (pos.size() != N_POS) { fputs("Invalid number of parameters\n", stderr); fputs(usage, stderr); return EXIT_FAILURE; }
    try {
        Options opt;
        memset(&opt, 0, sizeof opt);
        opt.size = sizeof opt;
        opt.log_domain = (uint32_t)logDomain;
        opt.validate = (uint32_t)validate;
#ifdef UG_ULTRA
        const ugcli::UltraSpec spec = ugcli::readUltraSpec(pos[2]);
        opt.rand_indx = spec.randIndx;
        opt.round_signals = spec.roundSignals.data(); opt.n_round = spec.roundSignals.size();
        opt.final_signals = spec.finalSignals.data(); opt.n_final = spec.finalSignals.size();
        uint8_t* const deltaAt = opt.delta_round;                     // (delta_final follows it in the struct)
        static_assert(offsetof(Options, delta_final) == offsetof(Options, delta_round) + 32, "the two deltas side by side");
#else
        uint8_t* const deltaAt = opt.delta;
#endif
        if (delta.empty()) {
#ifdef UG_ULTRA
            fputs(TOOL ": no contribution: delta_round = delta_final = 1. ANYONE can forge proofs for this key until a contribution is applied.\n", stderr);
#else
            fputs("zkey_new: no contribution: delta = 1. ANYONE can forge proofs for this key until a contribution is applied.\n", stderr);
#endif
        } else if (delta == "draw") {
            opt.contribute = 2;
            fputs(TOOL ": a single-party phase 2 with no transcript: the key is sound only if this run's delta is gone and the .ptau is "
                  "honest, and `snarkjs zkey verify` will not accept it.\n", stderr);
        } else {
            opt.contribute = 1;
            ughost::FileMap d(delta);
#ifdef UG_ULTRA
            if (d.size() != DELTA_BYTES) throw std::invalid_argument("--delta: the file must hold 64 bytes (delta_round, delta_final: little-endian, below r, not 0)");
#else
            if (d.size() != DELTA_BYTES) throw std::invalid_argument("--delta: the file must hold 32 bytes (little-endian, below r, not 0)");
#endif
            memcpy(deltaAt, d.data(), DELTA_BYTES);
            fputs(TOOL ": a delta from a file: whoever can read that file forges proofs for this key.\n", stderr);
        }
        char message[1024] = {0};
        ughost::FileMap r1cs(pos[0]), ptau(pos[1]);
        uint64_t zbytes = 0, vmax = 0;
#ifdef UG_ULTRA
        const auto sizeCall = ug_ultra_setup_ptau_size;
        const auto runCall = ug_ultra_setup_ptau_run;
#else
        const auto sizeCall = ug_setup_ptau_size;
        const auto runCall = ug_setup_ptau_run;
#endif
        if (sizeCall(&opt, r1cs.data(), r1cs.size(), ptau.data(), ptau.size(), &zbytes, &vmax, message, sizeof(message) - 1) != UG_OK)
            throw std::runtime_error(message);
        std::vector<uint8_t> zkey(zbytes);
        std::vector<char> vkey(vmax);
        double ms[UG_SETUP_PTAU_PHASES];
        uint64_t vlen = 0;
        const int rc = runCall(&opt, r1cs.data(), r1cs.size(), ptau.data(), ptau.size(), (int)device, zkey.data(), zkey.size(), &zbytes,
                               vkey.data(), vkey.size(), &vlen, ms, message, sizeof(message) - 1);
        volatile uint8_t* w = deltaAt;
        for (size_t i = 0; i < DELTA_BYTES; i++) w[i] = 0;
        if (rc != UG_OK) throw std::runtime_error(message);
        ugcli::writeFile(pos[N_POS - 2], zkey.data(), zbytes);
        ugcli::writeFile(pos[N_POS - 1], vkey.data(), vlen);
        printf("key written: %llu bytes (parse %.1f | point check %.1f | G1 combinations %.1f | G2 combination %.1f | delta %.1f | assembly %.1f ms)\n",
               (unsigned long long)zbytes, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
        return EXIT_SUCCESS;
    } catch (const std::exception& e) {
        fprintf(stderr, "Error: %s\n", e.what());
    }
    return EXIT_FAILURE;
}
