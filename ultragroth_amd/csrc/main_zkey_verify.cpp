// main_zkey_verify.cpp -- `zkey_verify <circuit.r1cs> <prepared.ptau> <key.zkey> [--validate 1|2] [--device d]`
// Is this Groth16 key the one its circuit and the powers-of-tau file give under one delta? On top of include/ultragroth_hip.h
// (ug_zkey_verify_run). Exit code 0: valid, 1: invalid, 2: refused (a file that cannot be read, sizes that do not belong
// together, a bad point). One line on stdout, the message on stderr. The three files are mapped, never read whole.
//   --validate 2     every point's field range and curve, every G2 point's subgroup (the default, and the only level whose
//                    answer is "valid"); 1 leaves the subgroup out, for timing: the line then says so
//   --device d       -1 runs on host threads (default: ULTRAGROTH_DEVICE, else 0)
// Not checked: who contributed (section 10's transcript, beacons, the .ptau's own ceremony); UltraGroth keys are refused.
//
// Built with -DUG_ULTRA: `zkey_verify_ultra <circuit.r1cs> <prepared.ptau> <key.zkey> [--spec spec.json] [the same options]`, the
// same question for an UltraGroth key (ug_ultra_zkey_verify_run), sections 2 - 12. --spec: dev_setup --ultra's file; the key's
// rand_indx and lists must then equal it. Without it the key's own rounds are taken as they are: who chose them is not checked.
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
#define TOOL "zkey_verify_ultra"
#define SPEC_USAGE " [--spec spec.json]"
constexpr int LAST_SECTION = 12;
#else
#define TOOL "zkey_verify"
#define SPEC_USAGE ""
constexpr int LAST_SECTION = 9;
#endif

int main(int argc, char** argv) {
    const char* usage = "Usage: " TOOL " <circuit.r1cs> <prepared.ptau> <key.zkey>" SPEC_USAGE " [--validate 1|2] [--device d]\n";
    std::vector<std::string> pos;
    long validate = 2, device = ugcli::defaultDevice();
    std::vector<ugcli::Option> options = {ugcli::validateOption(&validate, 1, "Error: --validate takes 1 or 2\n"), ugcli::deviceOption(&device)};
#ifdef UG_ULTRA
    std::string specPath;
    options.push_back(ugcli::textOption("--spec", &specPath));
#endif
    if (!ugcli::parseArgs(argc, argv, options, usage, pos)) return 2;
    if (pos.size() != 3) { fputs("Invalid number of parameters\n", stderr); fputs(usage, stderr); return 2; }
    try {
#ifdef UG_ULTRA
        ug_ultra_zkey_verify_options opt;
        const auto runCall = ug_ultra_zkey_verify_run;
#else
        ug_zkey_verify_options opt;
        const auto runCall = ug_zkey_verify_run;
#endif
        memset(&opt, 0, sizeof opt);
        opt.size = sizeof opt;
        opt.validate = (uint32_t)validate;
#ifdef UG_ULTRA
        ugcli::UltraSpec spec;
        if (!specPath.empty()) {
            spec = ugcli::readUltraSpec(specPath);
            opt.check_spec = 1;
            opt.rand_indx = spec.randIndx;
            opt.round_signals = spec.roundSignals.data(); opt.n_round = spec.roundSignals.size();
            opt.final_signals = spec.finalSignals.data(); opt.n_final = spec.finalSignals.size();
        }
#endif
        char message[1024] = {0};
        ughost::FileMap r1cs(pos[0]), ptau(pos[1]), zkey(pos[2]);
        ug_zkey_verify_report rep;
        double ms[UG_ZKEY_VERIFY_PHASES];
        const int rc = runCall(&opt, r1cs.data(), r1cs.size(), ptau.data(), ptau.size(), zkey.data(), zkey.size(), (int)device, &rep, ms, message,
                               sizeof(message) - 1);
        if (rc == UG_ERROR) {
            printf("refused\n");
            fprintf(stderr, "Error: %s\n", message);
            return 2;
        }
        std::string sections;
        for (int id = 2; id <= LAST_SECTION; id++)
            if (rep.failed_sections & (1u << id)) sections += (sections.empty() ? "" : ", ") + std::to_string(id);
        const std::string verdict = rc == UG_ZKEY_INVALID ? "invalid: sections " + sections
                                  : rep.subgroup_checked ? std::string("valid") : std::string("relations hold, subgroup not checked");
        printf("%s (parse %.1f | point check %.1f | weights %.1f | fold %.1f, its kernel %.3f | slice products %.1f | key products %.1f | "
               "H products %.1f | pairings %.1f ms; peak device memory %.1f MiB)\n",
               verdict.c_str(), ms[0], ms[1], ms[2], ms[3], rep.fold_kernel_ms, ms[4], ms[5], ms[6], ms[7], rep.peak_device_bytes / 1048576.0);
        if (rc == UG_ZKEY_INVALID) {
            fprintf(stderr, "%s\n", message);
            return 1;
        }
        return 0;
    } catch (const std::exception& e) {
        printf("refused\n");
        fprintf(stderr, "Error: %s\n", e.what());
    }
    return 2;
}
