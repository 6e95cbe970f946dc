// fuzz_sampling_parsers.cpp -- the header parser and the progressive decoder with any_sampling on, under AddressSanitizer / UBSan on
// the CPU: every seed file as it is (it must parse with the flag, with consistent geometry, and be refused without it), then mutated
// copies (bytes flipped, sampling factors and sizes rewritten, truncations), which may fail but must not touch memory
// they do not own.  What the parsers return sizes device buffers, so the numbers are checked against each other as the caller would
// use them.
// usage: fuzz_sampling_parsers <seed file>... <iterations>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libultrahdr_dev_amd/csrc/uhdr_jpeg.h"

using namespace uhdr::jpeg;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

static bool consistent(const DecInfo& in) {
  if (in.w <= 0 || in.h <= 0) return false;
  if (in.gray ? (in.hs != 1 || in.vs != 1) : (in.hs < 1 || in.hs > 2 || in.vs < 1 || in.vs > 2)) return false;
  if (in.w > 8192 || in.h > 8192) return true;   // refused by the callers before anything is sized
  const uint64_t mcus = (uint64_t)((in.w + 8 * in.hs - 1) / (8 * in.hs)) * (uint64_t)((in.h + 8 * in.vs - 1) / (8 * in.vs));
  const uint64_t nblk = mcus * (in.gray ? 1u : (uint64_t)(in.hs * in.vs + 2));
  if (in.progressive) return in.coef.size() == nblk * 64u && in.scan_bytes == 0;
  return in.restart_interval == 0 || in.interval_start.size() == (mcus + in.restart_interval - 1) / in.restart_interval;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::vector<std::vector<uint8_t>> seeds;
  for (int i = 1; i + 1 < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
    std::vector<uint8_t> d;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + n);
    fclose(f);
    DecInfo in;
    if (parse_header(d.data(), d.size(), &in, true) != 0 || !consistent(in)) { fprintf(stderr, "seed %s does not parse\n", argv[i]); return 1; }
    DecInfo strict;
    if (!in.gray && !(in.hs == 2 && in.vs == 2) && parse_header(d.data(), d.size(), &strict, false) == 0) { fprintf(stderr, "seed %s: accepted without the flag\n", argv[i]); return 1; }
    seeds.push_back(std::move(d));
  }
  const long iters = atol(argv[argc - 1]);
  long ok = 0;
  for (long it = 0; it < iters; ++it) {
    const std::vector<uint8_t>& s = seeds[rnd() % seeds.size()];
    std::vector<uint8_t> d(s.begin(), s.end());   // (exact size: ASan sees a read one byte past the file)
    const uint32_t kind = rnd() % 4u;
    if (kind == 0) { for (uint32_t k = 0, n = 1 + rnd() % 4u; k < n; ++k) d[rnd() % d.size()] = (uint8_t)rnd(); }
    else if (kind == 1) { d.resize(1 + rnd() % d.size()); }
    else {   // the frame header: sampling factors, component count, size
      for (size_t p = 2; p + 12 < d.size(); ++p)
        if (d[p] == 0xFF && (d[p + 1] == 0xC0 || d[p + 1] == 0xC2)) {
          const uint32_t what = rnd() % 4u;
          if (what == 0) d[p + 11 + 3 * (rnd() % 3u)] = (uint8_t)(((1 + rnd() % 4u) << 4) | (1 + rnd() % 4u));
          else if (what == 1) d[p + 9] = (uint8_t)(rnd() % 5u);
          else if (what == 2) { d[p + 5] = (uint8_t)(rnd() % 3u); d[p + 6] = (uint8_t)rnd(); }
          else { d[p + 7] = (uint8_t)(rnd() % 3u); d[p + 8] = (uint8_t)rnd(); }
          break;
        }
    }
    DecInfo in;
    if (parse_header(d.data(), d.size(), &in, (rnd() & 1u) != 0) == 0) {
      if (!consistent(in)) { fprintf(stderr, "iteration %ld: inconsistent geometry\n", it); return 1; }
      ++ok;
    }
  }
  printf("fuzz ok: %ld iterations, %ld parsed\n", iters, ok);
  return 0;
}
