// The progressive-JPEG host code under AddressSanitizer + UndefinedBehaviorSanitizer: the planner
// reidmi_jpeg_plan_ex with REIDMI_JPEG_PROGRESSIVE (jpeg.hip: the marker walk of the whole file,
// the scan table) and jpeg_core.h's progressive_decode (the lines jpeg_progressive_kernel runs,
// compiled for the host as in tools/jpeg_host_check.hip), as one standalone executable in the
// style of tools/jpeg_asan_main.hip (no sanitizer runtime preloaded into Python; never on a GPU).
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all -fno-omit-frame-pointer -g \
//         -Imultimodal-reid_amd/csrc -Iinclude tools/jpeg_prog_asan_main.hip -o jpeg_prog_asan
// tests/test_jpeg_progressive.py feeds it the parity files and their random mutations and
// compares its answers with the unsanitised library.  Not part of the product library.
//
// stdin:  int64 B, int64 offsets[B + 1], file bytes.
// stdout: int32 plan status[B], int64 meta[3 B], int64 info[10], int32 err[B],
//         uint8 pixels[info[2]].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "capi.hip"
#include "jpeg.hip"
#include "../../tools/jpeg_host_check.hip"

static void die(const char* m) {
    fprintf(stderr, "jpeg_prog_asan: %s\n", m);
    exit(2);
}

int main() {
    int64_t B;
    if (fread(&B, 8, 1, stdin) != 1 || B < 0 || B > (1 << 24)) die("bad count");
    std::vector<int64_t> off((size_t)B + 1);
    if (fread(off.data(), 8, off.size(), stdin) != off.size()) die("short offsets");
    const size_t nbytes = (size_t)off[(size_t)B];
    // exactly sized: a read past the last file's end is an ASan error
    uint8_t* files = (uint8_t*)malloc(nbytes ? nbytes : 1);
    if (nbytes && fread(files, 1, nbytes, stdin) != nbytes) die("short files");
    std::vector<int64_t> meta((size_t)(3 * B + 3)), info(10);
    std::vector<int32_t> status((size_t)B + 1);
    const int flags = REIDMI_JPEG_PROGRESSIVE;
    if (reidmi_jpeg_plan_ex(files, off.data(), B, flags, nullptr, 0, meta.data(), status.data(), info.data()) != 0)
        die(reidmi_last_error());
    // exactly sized too: the scan table and the list of progressive images end the blob
    uint8_t* plan = (uint8_t*)malloc((size_t)info[0] ? (size_t)info[0] : 1);
    if (reidmi_jpeg_plan_ex(files, off.data(), B, flags, plan, info[0], meta.data(), status.data(), info.data()) != 0)
        die(reidmi_last_error());
    std::vector<uint8_t> out((size_t)info[2] + 1);
    std::vector<int32_t> err((size_t)B + 1);
    host_decode(files, plan, info.data(), out.data(), err.data(), false);
    fwrite(status.data(), 4, (size_t)B, stdout);
    fwrite(meta.data(), 8, (size_t)(3 * B), stdout);
    fwrite(info.data(), 8, 10, stdout);
    fwrite(err.data(), 4, (size_t)B, stdout);
    fwrite(out.data(), 1, (size_t)info[2], stdout);
    fflush(stdout);
    free(plan);
    free(files);
    return 0;
}
