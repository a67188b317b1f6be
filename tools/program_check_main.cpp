// Host-sanitizer driver of the loader's program check: reads every blob file named on the command line and calls
// ta_program_check on it (the kind is taken from the blob's own header, so the check goes as deep as the blob lets it).
// The loader parses bytes it did not write; this runs it under AddressSanitizer + UBSan on a machine without a GPU -- the
// check makes no HIP call.  Stand-alone: never loaded into python, never run on a GPU machine.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -x hip tools/program_check_main.cpp terran_amd/csrc/model_load.hip terran_amd/csrc/runtime.hip -o /tmp/program_check
//   python -m tests.test_program_check_cpu --dump-blobs /tmp/blobs
//   /tmp/program_check /tmp/blobs/*.tam
//
// Prints one line per verdict class and exits 0 when every call returned (a sanitizer report aborts the run).
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/terran_amd.h"

void ta_pose_free_big(ta_ctx*) {}   // runtime.hip's context teardown calls into the pose unit; no context is ever made here

int main(int argc, char** argv) {
  int accepted = 0, refused = 0;
  for (int i = 1; i < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[i]);
      return 2;
    }
    std::vector<char> blob;
    char chunk[65536];
    for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) blob.insert(blob.end(), chunk, chunk + n);
    fclose(f);
    // an exact-size heap copy: a read one byte past the blob is a report, not a read of vector slack
    char* exact = new char[blob.size()];
    if (!blob.empty()) memcpy(exact, blob.data(), blob.size());
    int kind = 0;
    if (blob.size() >= 12) memcpy(&kind, exact + 8, 4);
    char msg[256];
    const int rc = ta_program_check(kind, exact, blob.size(), msg, sizeof(msg));
    delete[] exact;
    if (rc == TA_OK) {
      ++accepted;
    } else if (rc == TA_E_INVALID && msg[0]) {
      ++refused;
    } else {
      fprintf(stderr, "%s: unexpected result %d '%s'\n", argv[i], rc, msg);
      return 1;
    }
  }
  printf("%d blobs: %d accepted, %d refused with a message\n", argc - 1, accepted, refused);
  return 0;
}
