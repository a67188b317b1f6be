// The host half of ta_gallery_cluster (terran_amd/csrc/gallery_cluster_host.h) on its own, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -I terran_amd/csrc tests/native/cluster_host_check.cpp -o check && ./check
// Exit status 0 and "ok" if every check holds.
#include <string.h>

#include "gallery_cluster_host.h"

static int failures = 0;
#define CHECK(x)                                             \
  do {                                                       \
    if (!(x)) {                                              \
      fprintf(stderr, "line %d: %s\n", __LINE__, #x);        \
      ++failures;                                            \
    }                                                        \
  } while (0)

int main() {
  char msg[192];
  int32_t out[8];
  // argument checks
  CHECK(gal_cluster_check(0.5f, 1, 8, out, msg, sizeof(msg)) == nullptr);
  CHECK(gal_cluster_check(0.5f, 1, 0, nullptr, msg, sizeof(msg)) == nullptr);                 // empty: no output needed
  CHECK(gal_cluster_check(0.5f, 0, 8, out, msg, sizeof(msg)) && strstr(msg, "min_samples"));
  CHECK(gal_cluster_check(0.5f, -3, 8, out, msg, sizeof(msg)) != nullptr);
  CHECK(gal_cluster_check(NAN, 1, 8, out, msg, sizeof(msg)) && strstr(msg, "finite"));
  CHECK(gal_cluster_check(INFINITY, 1, 8, out, msg, sizeof(msg)) != nullptr);
  CHECK(gal_cluster_check(-INFINITY, 1, 8, out, msg, sizeof(msg)) != nullptr);
  CHECK(gal_cluster_check(0.5f, 1, 8, nullptr, msg, sizeof(msg)) && strstr(msg, "null"));
  CHECK(gal_cluster_check(0.5f, 1, GAL_CLUSTER_MAX_ROWS, out, msg, sizeof(msg)) == nullptr);
  CHECK(gal_cluster_check(0.5f, 1, GAL_CLUSTER_MAX_ROWS + 1, out, msg, sizeof(msg)) && strstr(msg, "262144") && strstr(msg, "2^18"));
  char tiny[8];                                                                                // a short buffer is not overrun
  CHECK(gal_cluster_check(0.5f, 0, 8, out, tiny, sizeof(tiny)) == tiny && strlen(tiny) == 7);
  setenv("TA_GALLERY_CLUSTER_MAX_ROWS", "5", 1);
  CHECK(gal_cluster_limit() == 5);
  CHECK(gal_cluster_check(0.5f, 1, 6, out, msg, sizeof(msg)) && strstr(msg, "the 5 that"));
  CHECK(gal_cluster_check(0.5f, 1, 5, out, msg, sizeof(msg)) == nullptr);
  setenv("TA_GALLERY_CLUSTER_MAX_ROWS", "999999999", 1);                                       // the switch only lowers
  CHECK(gal_cluster_limit() == GAL_CLUSTER_MAX_ROWS);
  setenv("TA_GALLERY_CLUSTER_MAX_ROWS", "-4", 1);
  CHECK(gal_cluster_limit() == GAL_CLUSTER_MAX_ROWS);
  unsetenv("TA_GALLERY_CLUSTER_MAX_ROWS");

  // renumbering: roots 2 and 5 -> clusters 0 and 1; row 0 is a border row of the later root, rows 3 and 7 are noise
  const int32_t root[8] = {5, 2, 2, -1, 5, 5, 2, -1};
  CHECK(gal_renumber(root, 8, out) == 2);
  const int32_t want[8] = {1, 0, 0, -1, 1, 1, 0, -1};
  CHECK(memcmp(out, want, sizeof(want)) == 0);
  CHECK(gal_renumber(root, 0, out) == 0);
  const int32_t noise[3] = {-1, -1, -1};
  CHECK(gal_renumber(noise, 3, out) == 0 && out[0] == -1 && out[2] == -1);
  const int32_t beyond[3] = {0, 3, 0};                                                         // a label past the end
  CHECK(gal_renumber(beyond, 3, out) == -1);
  const int32_t no_root[3] = {1, 2, 2};                                                        // row 0 points at row 1, which is no root
  CHECK(gal_renumber(no_root, 3, out) == -1);
  const int32_t sentinel[2] = {0, 0x7fffffff};
  CHECK(gal_renumber(sentinel, 2, out) == -1);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
