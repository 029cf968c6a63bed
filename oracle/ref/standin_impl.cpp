// The parts of the CUDA stand-in (standin/cuda_runtime.h) that need storage
// or are too long for a header.
#include <cuda_runtime.h>

thread_local uint3 threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

namespace vro_ref
{
static int pick(bool takeMax, int a, int b) { return takeMax ? (a > b ? a : b) : (a < b ? a : b); }

int ptxInt(const char *text, const int *in, int nIn)
{
  // predicate ballot of one lane: bit 0 is the lane's own predicate
  if(std::strstr(text, "vote.ballot.b32") && std::strstr(text, "setp.ge.s32") && nIn == 1)
    return in[0] >= 0 ? 1 : 0;
  // v{min,max}.s32.s32.s32.{min,max} d, a, b, c  =  op2(op1(a, b), c)
  for(int first = 0; first < 2; ++first)
    for(int second = 0; second < 2; ++second)
    {
      char op[48];
      std::snprintf(op, sizeof op, "v%s.s32.s32.s32.%s", first ? "max" : "min", second ? "max" : "min");
      if(std::strstr(text, op) && nIn == 3)
        return pick(second != 0, pick(first != 0, in[0], in[1]), in[2]);
    }
  std::fprintf(stderr, "vro_ref: no interpretation for PTX text: %s\n", text);
  std::abort();
}
}
