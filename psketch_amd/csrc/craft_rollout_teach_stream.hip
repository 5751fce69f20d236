// craft_rollout_teach_stream.hip — craft_rollout_teach_stream: rollout_teach_kernel's QUEUE
// instantiations (craft_rollout_teach.h), the teacher-labelled K-tick launch on the episode
// queue.  A translation unit of its own, so that the craft_rollout_teach kernels' unit compiles
// as before.
#include "craft_launch.h"
#include "craft_rollout_teach.h"

namespace craft {

hipError_t launch_rollout_teach_stream(int win, int nw, const SimView& v, const RolloutArgs& a, hipStream_t st) {
  return launch_rt<true>(win, nw, v, a, 0, st);
}

}  // namespace craft
