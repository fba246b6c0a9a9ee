// main_wtns_check.cpp -- `wtns_check <circuit.r1cs> <witness.wtns>`: does the witness satisfy every constraint of the circuit?
// On top of include/prover.h (ug_witness_check). Exit 0 and "witness ok: <m> constraints", or exit 1 with the message and the
// three values of the first failing constraint in decimal. ULTRAGROTH_DEVICE selects the device; -1 runs on host threads.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "host_util.hpp"
#include "../../include/prover.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        fputs("Invalid number of parameters\nUsage: wtns_check <circuit.r1cs> <witness.wtns>\n", stderr);
        return EXIT_FAILURE;
    }
    try {
        ughost::FileMap r1cs(argv[1]), wtns(argv[2]);
        const char* e = getenv("ULTRAGROTH_DEVICE");
        char message[1024] = {0};
        ug_witness_fault fault;
        const int rc = ug_witness_check(r1cs.data(), r1cs.size(), wtns.data(), wtns.size(), e ? atoi(e) : 0, &fault, message, sizeof(message) - 1);
        if (rc == PROVER_OK) {
            ughost::BinFile f(r1cs.data(), r1cs.size(), "r1cs", 1);
            printf("witness ok: %u constraints\n", ughost::loadR1csHeader(f).nConstraints);
            return EXIT_SUCCESS;
        }
        fprintf(stderr, "Error: %s\n", message);
        if (fault.failed)
            fprintf(stderr, "A.w = %s\nB.w = %s\nC.w = %s\n", ughost::toDecimal(fault.a).c_str(), ughost::toDecimal(fault.b).c_str(),
                    ughost::toDecimal(fault.c).c_str());
    } catch (const std::exception& e) {
        fprintf(stderr, "Error: %s\n", e.what());
    }
    return EXIT_FAILURE;
}
