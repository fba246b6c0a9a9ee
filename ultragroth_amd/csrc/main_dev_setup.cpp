// main_dev_setup.cpp -- `dev_setup <circuit.r1cs> <out.zkey> <out_vkey.json> [--trapdoor t.json] [--log-domain n] [--ultra spec.json]`
// A development setup on top of include/ultragroth_hip.h (ug_setup_*): a proving key and its verification key from the circuit
// and a KNOWN trapdoor. The result is a TEST key -- whoever knows the trapdoor forges proofs -- and every run says so on stderr.
//   --trapdoor t.json   {"tau", "alpha", "beta", "gamma", "delta_round", "delta_final"}: decimal strings (the keys of
//                       tests/golden/trapdoor/trapdoor.json). Without it one is drawn from OS entropy and written to
//                       <out.zkey>.trapdoor.json.
//   --ultra spec.json   protocol 1337: {"rand_indx": n, "round_signals": [...], "final_signals": [...]}
// ULTRAGROTH_DEVICE selects the device; -1 runs on host threads.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>
#include "cli_util.hpp"
#include "host_util.hpp"
#include "cli_spec.hpp"
#include "../../include/ultragroth_hip.h"

namespace {

const char* const NAMES[6] = {"tau", "alpha", "beta", "gamma", "delta_round", "delta_final"};

// decimal -> 32-byte little-endian, exactly: a value of 2^256 or more is an error, not a residue
void decimalToLe(uint8_t out[32], const std::string& s, const char* what) {
    if (s.empty()) throw std::invalid_argument(std::string(what) + ": not a number");
    uint32_t w[8] = {0};
    for (char ch : s) {
        if (ch < '0' || ch > '9') throw std::invalid_argument(std::string(what) + ": not a number");
        uint64_t carry = (uint64_t)(ch - '0');
        for (int i = 0; i < 8; i++) { carry += (uint64_t)w[i] * 10; w[i] = (uint32_t)carry; carry >>= 32; }
        if (carry) throw std::invalid_argument(std::string(what) + ": not below 2^256");
    }
    memcpy(out, w, 32);
}

}  // namespace

int main(int argc, char** argv) {
    const char* usage = "Usage: dev_setup <circuit.r1cs> <out.zkey> <out_vkey.json> [--trapdoor t.json] [--log-domain n] [--ultra spec.json]\n";
    fputs("dev_setup: this makes a TEST key from a known trapdoor. Whoever knows the trapdoor forges proofs: never use it where a proof must mean anything.\n", stderr);
    std::vector<std::string> pos;
    std::string trapdoorPath, ultraPath;
    long logDomain = 0;
    const std::vector<ugcli::Option> options = {ugcli::textOption("--trapdoor", &trapdoorPath), ugcli::textOption("--ultra", &ultraPath),
                                                ugcli::numberOption("--log-domain", &logDomain, 0, 64, "Error: --log-domain takes a number\n", true)};
    if (!ugcli::parseArgs(argc, argv, options, usage, pos)) return EXIT_FAILURE;
    if (pos.size() != 3) { fputs("Invalid number of parameters\n", stderr); fputs(usage, stderr); return EXIT_FAILURE; }
    try {
        ug_setup_options opt;
        memset(&opt, 0, sizeof opt);
        opt.size = sizeof opt;
        opt.protocol = 1;
        opt.log_domain = (uint32_t)logDomain;
        uint8_t* vals[6] = {opt.tau, opt.alpha, opt.beta, opt.gamma, opt.delta_round, opt.delta_final};
        char message[1024] = {0};
        if (!trapdoorPath.empty()) {
            const std::string text = ugcli::slurp(trapdoorPath);
            const ugv::JVal j = ugv::JParser(text.c_str()).parse_document();
            for (int i = 0; i < 6; i++) decimalToLe(vals[i], j.at(NAMES[i]).string(), NAMES[i]);
        } else {
            if (ug_setup_draw_trapdoor(&opt, message, sizeof(message) - 1) != UG_OK) throw std::runtime_error(message);
            std::string out = "{\n";
            for (int i = 0; i < 6; i++) out += std::string(" \"") + NAMES[i] + "\": \"" + ughost::toDecimal(vals[i]) + "\"" + (i < 5 ? ",\n" : "\n");
            out += "}\n";
            ugcli::writeFile(pos[1] + ".trapdoor.json", out.data(), out.size());
            fprintf(stderr, "dev_setup: the trapdoor (the toxic waste of this TEST key) is in %s.trapdoor.json\n", pos[1].c_str());
        }
        ugcli::UltraSpec spec;
        if (!ultraPath.empty()) {
            spec = ugcli::readUltraSpec(ultraPath);
            opt.protocol = 1337;
            opt.rand_indx = spec.randIndx;
            opt.round_signals = spec.roundSignals.data(); opt.n_round = spec.roundSignals.size();
            opt.final_signals = spec.finalSignals.data(); opt.n_final = spec.finalSignals.size();
        }
        ughost::FileMap r1cs(pos[0]);
        uint64_t zbytes = 0, vmax = 0;
        if (ug_setup_size(&opt, r1cs.data(), r1cs.size(), &zbytes, &vmax, message, sizeof(message) - 1) != UG_OK) throw std::runtime_error(message);
        std::vector<uint8_t> zkey(zbytes);
        std::vector<char> vkey(vmax);
        double ms[UG_SETUP_PHASES];
        uint64_t vlen = 0;
        if (ug_setup_run(&opt, r1cs.data(), r1cs.size(), (int)ugcli::defaultDevice(), zkey.data(), zkey.size(), &zbytes, vkey.data(), vkey.size(), &vlen, ms, message,
                         sizeof(message) - 1) != UG_OK)
            throw std::runtime_error(message);
        ugcli::writeFile(pos[1], zkey.data(), zbytes);
        ugcli::writeFile(pos[2], vkey.data(), vlen);
        printf("test key written: %llu bytes (parse %.1f | lagrange %.1f | products %.1f | G1 %.1f | G2 %.1f | assembly %.1f ms)\n",
               (unsigned long long)zbytes, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
        return EXIT_SUCCESS;
    } catch (const std::exception& e) {
        fprintf(stderr, "Error: %s\n", e.what());
    }
    return EXIT_FAILURE;
}
