// main_zkey_verify.cpp -- `zkey_verify <circuit.r1cs> <prepared.ptau> <key.zkey> [--validate 1|2] [--device d] [--locate [--max-listed n]]`
// Is this Groth16 key the one its circuit and the powers-of-tau file give under one delta? On top of include/ultragroth_hip.h
// (ug_zkey_verify_run). Exit code 0: valid, 1: invalid, 2: refused (a file that cannot be read, sizes that do not belong
// together, a bad point). One line on stdout, the message on stderr. The three files are mapped, never read whole.
//   --validate 2     every point's field range and curve, every G2 point's subgroup (the default, and the only level whose
//                    answer is "valid"); 1 leaves the subgroup out, for timing: the line then says so
//   --device d       -1 runs on host threads (default: ULTRAGROTH_DEVICE, else 0)
//   --locate         an invalid key: one more line on stdout per failing point section (3, 5, 6, 7, the C sections, H) that names its
//                    wrong records (ug_zkey_locate_run), e.g. "section 8: 2 of 1 048 575 records wrong: 17, 40211". Without the flag
//                    output and exit codes are what they were. --max-listed n: at most n records per line (default 16, up to 1024)
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

// 1048575 -> "1 048 575"
static std::string grouped(uint64_t v) {
    std::string d = std::to_string(v), out;
    for (size_t i = 0; i < d.size(); i++) {
        if (i && (d.size() - i) % 3 == 0) out += ' ';
        out += d[i];
    }
    return out;
}
// one line per located section
static void printLocated(const ug_zkey_locate_report& located) {
    for (uint32_t s = 0; s < located.n_sections; s++) {
        const ug_zkey_locate_section& e = located.section[s];
        // (not exact: blocks fail beyond the resolved ones, so no resolved block is the short last one: each has 256 records)
        if (!e.exact && e.resolved_blocks && e.bad_records == e.resolved_blocks * 256) {
            printf("section %u: every resolved block fails (%s of %s resolved): not a few bad records\n", e.section, grouped(e.resolved_blocks).c_str(),
                   grouped(e.bad_blocks).c_str());
            continue;
        }
        std::string list;
        for (uint32_t i = 0; i < e.n_listed; i++) list += (i ? ", " : "") + std::to_string(e.index[i]);
        if (e.n_listed < e.bad_records) list += ", ...";
        const std::string part = e.exact ? "" : " in the " + grouped(e.resolved_blocks) + " of " + grouped(e.bad_blocks) + " failing blocks that were resolved";
        printf("section %u: %s of %s records wrong%s: %s\n", e.section, grouped(e.bad_records).c_str(), grouped(e.records).c_str(), part.c_str(),
               list.c_str());
    }
}

int main(int argc, char** argv) {
    const char* usage = "Usage: " TOOL " <circuit.r1cs> <prepared.ptau> <key.zkey>" SPEC_USAGE " [--validate 1|2] [--device d] [--locate [--max-listed n]]\n";
    std::vector<std::string> pos;
    long validate = 2, device = ugcli::defaultDevice(), maxListed = 16;
    bool locate = false;
    std::vector<ugcli::Option> options = {ugcli::validateOption(&validate, 1, "Error: --validate takes 1 or 2\n"), ugcli::deviceOption(&device),
                                          ugcli::flagOption("--locate", &locate),
                                          ugcli::numberOption("--max-listed", &maxListed, 1, UG_ZKEY_LOCATE_LISTED, "Error: --max-listed takes 1 to 1024\n")};
#ifdef UG_ULTRA
    std::string specPath;
    options.push_back(ugcli::textOption("--spec", &specPath));
#endif
    if (!ugcli::parseArgs(argc, argv, options, usage, pos)) return 2;
    if (pos.size() != 3) { fputs("Invalid number of parameters\n", stderr); fputs(usage, stderr); return 2; }
    try {
        // (the locate options hold the verify options' fields, then two more: one struct serves both calls, under the size of each)
#ifdef UG_ULTRA
        ug_ultra_zkey_locate_options opt;
        ug_ultra_zkey_verify_options plain;
        const auto runCall = ug_ultra_zkey_verify_run;
        const auto locateCall = ug_ultra_zkey_locate_run;
#else
        ug_zkey_locate_options opt;
        ug_zkey_verify_options plain;
        const auto runCall = ug_zkey_verify_run;
        const auto locateCall = ug_zkey_locate_run;
#endif
        memset(&opt, 0, sizeof opt);
        opt.size = sizeof opt;
        opt.validate = (uint32_t)validate;
        opt.max_listed = (uint32_t)maxListed;
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
        std::vector<ug_zkey_locate_report> located(locate ? 1 : 0);
        int rc;
        if (locate) {
            rc = locateCall(&opt, r1cs.data(), r1cs.size(), ptau.data(), ptau.size(), zkey.data(), zkey.size(), (int)device, &rep, located.data(), ms,
                            message, sizeof(message) - 1);
        } else {
            memcpy(&plain, &opt, sizeof plain);
            plain.size = sizeof plain;
            rc = runCall(&plain, r1cs.data(), r1cs.size(), ptau.data(), ptau.size(), zkey.data(), zkey.size(), (int)device, &rep, ms, message,
                         sizeof(message) - 1);
        }
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
            if (locate) printLocated(located[0]);
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
