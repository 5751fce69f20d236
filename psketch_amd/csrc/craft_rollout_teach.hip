// craft_rollout_teach.hip — launches of the teacher-labelled K-tick rollout kernel
// (craft_rollout_teach.h), one instantiation per window and BFS word count.
#include "craft_launch.h"
#include "craft_rollout_teach.h"

namespace craft {

hipError_t launch_rollout_teach(int win, int nw, const SimView& v, const RolloutArgs& a, hipStream_t st) {
#ifdef CRAFT_STAMPS
  return launch_rt<false>(win, nw, v, a, 512, st);     // + the stamp sums
#else
  return launch_rt<false>(win, nw, v, a, 0, st);
#endif
}

}  // namespace craft
