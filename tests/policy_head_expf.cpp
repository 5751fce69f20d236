// A stand-alone check of the CPU variant's craft_expf (include/craft.h "The head rule"), built and
// run by tests/test_policy_head_cpu.py: the library's translation unit is included as it is, so
// the function measured is the one the library runs and no test hook is exported.  Prints the
// largest relative error against float64 exp over every 1021st float32 of [-80, 0] (the bit
// patterns 0x80000000 .. 0xC2A00000), the argument where it occurs, and the smallest value.
#include "../psketch_amd/csrc/craft_cpu.cpp"

int main() {
  double worst = 0.0;
  float at = 0.0f, smallest = 1.0f;
  long count = 0;
  for (uint64_t u = 0x80000000ull; u <= 0xC2A00000ull; u += 1021) {
    const float x = bits_float((uint32_t)u);
    const float e = craft_expf(x);
    const double rel = std::fabs((double)e / std::exp((double)x) - 1.0);
    if (rel > worst) {
      worst = rel;
      at = x;
    }
    if (e < smallest) smallest = e;
    ++count;
  }
  // -80 itself, the clamp's value
  const float e80 = craft_expf(-80.0f);
  const double rel80 = std::fabs((double)e80 / std::exp(-80.0) - 1.0);
  std::printf("count %ld max_rel %.6e at %.9g rel_at_minus_80 %.6e smallest %.9g\n", count, worst, (double)at, rel80,
              (double)(e80 < smallest ? e80 : smallest));
  return 0;
}
