// Host program of tests/test_candidate_radius_table.py: the radius decision of magnify_amd/csrc/mg_radius.h against
// the square root it replaces, on EVERY float32 s from 0 to the first value above (max_r + 1)^2, and on NaN, +inf and -0.
//   candidate_radius_main MIN_R MAX_R
// For every s the decision is made three times: with sqrtf(s) as the guess and with the floats one ulp below and above
// it (the kernel's guess is the hardware's 1-ulp square root).  Range test and layer must be those of
// min_r <= sqrtf(s) <= max_r and rintf(sqrtf(s)) - min_r.  Prints "checked N" and exits 0, or the first mismatches and 1.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../magnify_amd/csrc/mg_radius.h"

static uint32_t bits_of(float f) {
  uint32_t b;
  memcpy(&b, &f, sizeof b);
  return b;
}

static int failures = 0;

static void check(float s, const MgRadiusTable& tab) {
  volatile float vs = s;
  volatile float vroot = sqrtf(vs);
  const float root = vroot;
  const bool in_range = root >= (float)tab.min_r && root <= (float)tab.max_r;
  const int want = in_range ? (int)rintf(root) - tab.min_r : -1;
  float guesses[3] = {root, root, root};
  if (root == root && !isinf(root)) {
    guesses[1] = nextafterf(root, -INFINITY);
    guesses[2] = nextafterf(root, INFINITY);
  }
  for (float guess : guesses) {
    const int got = mg_radius_layer(s, guess, tab.lo, tab.hi, tab.t, tab.min_r, tab.max_r);
    if (got != want && failures++ < 10)
      printf("s = %a (0x%08x), guess %a: layer %d, want %d\n", (double)s, bits_of(s), (double)guess, got, want);
  }
}

// candidate_radius_main sum: the image coordinate of a centre, (float)((double)c + (double)p0) in the reference, against
// the single float32 add the key-only kernel makes (mg_circles.hip: image_coord_f32) -- every 611th float32 c of either
// sign (a stride coprime to the mantissa patterns), the floats next to each power of two, and p0 over the small
// coordinates, the powers of two and their neighbours up to 65535.
static int check_sums() {
  int p0s[64], n = 0;
  for (int p = 0; p <= 4; ++p) p0s[n++] = p;
  for (int k = 3; k <= 16; ++k) p0s[n++] = (1 << k) - 1, p0s[n++] = k < 16 ? (1 << k) : 65534, p0s[n++] = k < 16 ? (1 << k) + 1 : 43691;
  unsigned long long checked = 0;
  auto one = [&](uint32_t b) {
    const float c = mg_radius_from_bits(b);
    if (c != c) return;  // (a NaN stays a NaN either way; its payload is not compared)
    for (int i = 0; i < n; ++i) {
      volatile double wide = (double)c + (double)p0s[i];
      volatile float want = (float)wide;
      volatile float got = c + (float)p0s[i];
      const float w = want, g = got;
      ++checked;
      if (bits_of(w) != bits_of(g) && failures++ < 10) printf("c = %a, p0 = %d: %a, want %a\n", (double)c, p0s[i], (double)g, (double)w);
    }
  };
  for (uint64_t b = 0; b <= 0xFFFFFFFFull; b += 611) one((uint32_t)b);
  for (uint32_t e = 1; e < 255; ++e)
    for (uint32_t sign = 0; sign < 2; ++sign)
      for (int d = -2; d <= 2; ++d) one((sign << 31 | e << 23) + (uint32_t)d);
  if (failures) {
    printf("%d mismatches\n", failures);
    return 1;
  }
  printf("checked %llu\n", checked);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "sum")) return check_sums();
  if (argc != 3) return 2;
  const int min_r = atoi(argv[1]), max_r = atoi(argv[2]);
  if (min_r < 0 || max_r < min_r || max_r - min_r >= MG_RADIUS_MAX_LAYERS) return 2;
  MgRadiusTable tab;
  mg_radius_table(min_r, max_r, &tab);
  const float end = nextafterf((float)(max_r + 1) * (float)(max_r + 1), INFINITY);
  const uint32_t last = bits_of(end);
  for (uint32_t b = 0;; ++b) {
    check(mg_radius_from_bits(b), tab);
    if (b == last) break;
  }
  check(NAN, tab);
  check(-NAN, tab);
  check(INFINITY, tab);
  check(-0.0f, tab);
  check(3.0e38f, tab);
  if (failures) {
    printf("%d mismatches\n", failures);
    return 1;
  }
  printf("checked %u\n", last + 6u);
  return 0;
}
