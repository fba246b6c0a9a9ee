// main_ptau_prepare.cpp -- `ptau_prepare <in.ptau> <out.ptau> [--power p] [--validate 0|1|2] [--device d]`
//                          `ptau_prepare --check <prepared.ptau> [--validate 0|1|2] [--device d]`
// Prepares a powers-of-tau file for phase 2 on top of include/ultragroth_hip.h (ug_ptau_prepare_*): sections 12 - 15, the Lagrange
// forms, from the powers of sections 2 - 5 -- what `snarkjs powersoftau prepare phase2` does. --check recomputes the sections of a
// prepared file and compares them with its own, which zkey_new takes on trust.
//   --power p        cut the file to power p first (a 2^28 ceremony for a 2^20 circuit)
//   --device d       -1 runs on host threads (default: ULTRAGROTH_DEVICE, else 0)
// Input and output are mapped, never read whole; the output is created at its final size. Transcripts, beacons and verifying the
// ceremony's own contributions are out of scope.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <stdexcept>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <system_error>
#include <unistd.h>
#include <vector>
#include "cli_util.hpp"
#include "host_util.hpp"
#include "../../include/ultragroth_hip.h"

namespace {

// true when both paths name one existing file: creating the output would truncate the input under its own mapping
bool sameFile(const std::string& a, const std::string& b) {
    struct stat sa, sb;
    if (stat(a.c_str(), &sa) == -1 || stat(b.c_str(), &sb) == -1) return false;
    return sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

// a new file of `size` bytes, mapped for writing
class OutMap {
public:
    OutMap(const std::string& path, uint64_t size) : path_(path), size_(size) {
        fd_ = open(path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
        if (fd_ == -1) throw std::system_error(errno, std::generic_category(), "open " + path);
        if (ftruncate(fd_, (off_t)size) == -1) { const int e = errno; close(fd_); unlink(path.c_str()); throw std::system_error(e, std::generic_category(), "ftruncate"); }
        addr_ = mmap(nullptr, size ? size : 1, PROT_READ | PROT_WRITE, MAP_SHARED, fd_, 0);
        if (addr_ == MAP_FAILED) { const int e = errno; close(fd_); unlink(path.c_str()); throw std::system_error(e, std::generic_category(), "mmap"); }
    }
    ~OutMap() {
        munmap(addr_, size_ ? size_ : 1);
        close(fd_);
        if (!keep_) unlink(path_.c_str());       // (a run that failed leaves no half-written file)
    }
    void* data() const { return addr_; }
    void keep() {
        if (msync(addr_, size_, MS_SYNC) == -1) throw std::system_error(errno, std::generic_category(), "msync");
        keep_ = true;
    }
    OutMap(const OutMap&) = delete;
    OutMap& operator=(const OutMap&) = delete;
private:
    std::string path_;
    uint64_t size_;
    void* addr_ = nullptr;
    int fd_ = -1;
    bool keep_ = false;
};

}  // namespace

int main(int argc, char** argv) {
    const char* usage = "Usage: ptau_prepare <in.ptau> <out.ptau> [--power p] [--validate 0|1|2] [--device d]\n"
                        "       ptau_prepare --check <prepared.ptau> [--validate 0|1|2] [--device d]\n";
    std::vector<std::string> pos;
    long power = 0, validate = 1, device = ugcli::defaultDevice();
    bool check = false;
    const std::vector<ugcli::Option> options = {ugcli::flagOption("--check", &check),
                                                ugcli::numberOption("--power", &power, 1, 28, "Error: --power takes a power from 1 to 28\n"),
                                                ugcli::validateOption(&validate, 0, "Error: --validate takes 0, 1 or 2\n"), ugcli::deviceOption(&device)};
    if (!ugcli::parseArgs(argc, argv, options, usage, pos)) return EXIT_FAILURE;
    if (pos.size() != (check ? 1u : 2u)) { fputs("Invalid number of parameters\n", stderr); fputs(usage, stderr); return EXIT_FAILURE; }
    try {
        ug_ptau_prepare_options opt;
        memset(&opt, 0, sizeof opt);
        opt.size = sizeof opt;
        opt.power = (uint32_t)power;
        opt.validate = (uint32_t)validate;
        opt.mode = check ? 1 : 0;
        char message[1024] = {0};
        if (!check && sameFile(pos[0], pos[1])) throw std::invalid_argument("the output is the input file: give another path");
        ughost::FileMap in(pos[0]);
        uint64_t bytes = 0;
        if (ug_ptau_prepare_size(&opt, in.data(), in.size(), &bytes, message, sizeof(message) - 1) != UG_OK) throw std::runtime_error(message);
        double ms[UG_PTAU_PREPARE_PHASES];
        if (check) {
            if (ug_ptau_prepare_run(&opt, in.data(), in.size(), (int)device, nullptr, 0, nullptr, ms, message, sizeof(message) - 1) != UG_OK)
                throw std::runtime_error(message);
            printf("sections 12 - 15 are the Lagrange forms of sections 2 - 5 (parse %.1f | point check %.1f | G1 levels %.1f | G2 levels %.1f | "
                   "comparison %.1f ms)\n", ms[0], ms[1], ms[2], ms[3], ms[4]);
            return EXIT_SUCCESS;
        }
        OutMap out(pos[1], bytes);
        if (ug_ptau_prepare_run(&opt, in.data(), in.size(), (int)device, out.data(), bytes, &bytes, ms, message, sizeof(message) - 1) != UG_OK)
            throw std::runtime_error(message);
        out.keep();
        printf("prepared file written: %llu bytes (parse + copy %.1f | point check %.1f | G1 levels %.1f | G2 levels %.1f ms)\n",
               (unsigned long long)bytes, ms[0], ms[1], ms[2], ms[3]);
        return EXIT_SUCCESS;
    } catch (const std::exception& e) {
        fprintf(stderr, "Error: %s\n", e.what());
    }
    return EXIT_FAILURE;
}
