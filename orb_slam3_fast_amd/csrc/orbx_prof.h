// orbx_prof.h — the section clock of the measurement builds (make prof PROF_FLAGS=-D<flag>, output ../liborbx_prof.so; the
// scripts under tools/ load that library and parse the lines the kernels print).  This header is the only place where the
// build flags below meet the preprocessor: kernels see them as constexpr bools, and in the product build (none set) the
// clock is an empty object whose members compile to nothing.
//   OCT_PROF      sections of k_octree's selected workgroup (ORBX_OCTREE_PROF_LEVEL) and of its sort (OCT_NO_SORT_PRINT: not those)
//   OCT_WG_PROF   life of every (image, level) workgroup of k_octree
//   RS_PROF       phases of a few k_resize workgroups          RT_PROF   phases of one k_resize_tail band
//   ST_PROF       sections of k_stereo_sort / k_stereo_band    DET_PROF  life of a few k_detect cell-waves
//   DET_CLK       shader cycles per 10 ns tick in k_detect
#ifndef ORBX_PROF_H
#define ORBX_PROF_H
#include <hip/hip_runtime.h>

namespace orbx {

#ifdef OCT_PROF
constexpr bool kOctProf = true;
#else
constexpr bool kOctProf = false;
#endif
#ifdef OCT_NO_SORT_PRINT
constexpr bool kOctSortPrint = false;
#else
constexpr bool kOctSortPrint = kOctProf;
#endif
#ifdef OCT_WG_PROF
constexpr bool kOctWgProf = true;
#else
constexpr bool kOctWgProf = false;
#endif
#ifdef RS_PROF
constexpr bool kRsProf = true;
#else
constexpr bool kRsProf = false;
#endif
#ifdef RT_PROF
constexpr bool kRtProf = true;
#else
constexpr bool kRtProf = false;
#endif
#ifdef ST_PROF
constexpr bool kStProf = true;
#else
constexpr bool kStProf = false;
#endif
#ifdef DET_PROF
constexpr bool kDetProf = true;
#else
constexpr bool kDetProf = false;
#endif
#ifdef DET_CLK
constexpr bool kDetClk = true;
#else
constexpr bool kDetClk = false;
#endif

// Up to N time stamps of one thread, in 10 ns ticks of wall_clock64.  kOn == false: no storage worth the name, no code.
template <int N, bool kOn>
struct SectionClock {
  static constexpr bool on = kOn;
  long long t[kOn ? N : 1];
  int n = 0;
  __device__ __forceinline__ void mark() {
    if (n < N) t[n++] = wall_clock64();
  }
  __device__ __forceinline__ int total() const { return (int)(t[n - 1] - t[0]); }   // first to last mark
  // head (a printf format with its arguments), then the ticks between consecutive marks
  template <class... A>
  __device__ __forceinline__ void print(const char* head, A... a) const {
    if constexpr (kOn) {
      printf(head, a...);
      for (int i = 1; i < n; i++) printf(" %d", (int)(t[i] - t[i - 1]));
    }
  }
};
// A time stamp is taken with PROF_MARK(clk).  With the clock off the front end discards the statement, so the product
// kernel's IR is what it was without a clock.  (A call of an empty inline member is not the same thing: it stays in the IR
// until the inliner has run, and the passes in front of it then left k_octree and k_detect with another register allocation
// and block layout -- same resources, different text.)
#define PROF_MARK(clk) do { if constexpr (decltype(clk)::on) (clk).mark(); } while (0)

}  // namespace orbx
#endif
