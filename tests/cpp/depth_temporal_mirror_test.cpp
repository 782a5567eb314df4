// depth_temporal_mirror_test.cpp — SceneFlowConstructor::setDepthTemporal exists and forwards to mod_set_depth_temporal, without the
// library: mirror_calls_test.cpp's call recorder stands in for it (its ModContext, its stubs and its Rig; its main is renamed and not
// run), and the one stub it lacks is defined here.  tests/test_depth_temporal_abi.py reads the lines that begin with the call's name.
#define main mirror_calls_main
#include "mirror_calls_test.cpp"
#undef main

int mod_set_depth_temporal(ModContext *c, const ModDepthTemporal *f) {
  if (f) std::printf("mod_set_depth_temporal %g %g %g %d %d %d %d %d\n", f->alpha, f->delta_abs, f->delta_rel, f->hold, f->reserved[0], f->reserved[1], f->reserved[2], f->reserved[3]);
  else std::printf("mod_set_depth_temporal NULL\n");
  return c->code("mod_set_depth_temporal");
}

int main() {
  Rig r;
  const ModDepthTemporal f{0.25f, 0.5f, 0.125f, 3, {0, 0, 0, 0}};
  r.sfc.setDepthTemporal(&f);
  r.sfc.setDepthTemporal(nullptr);
  r.ctx.codes["mod_set_depth_temporal"] = {MOD_ERR_INVALID_ARGUMENT};     // a refusal becomes an exception, like every setter's
  try {
    r.sfc.setDepthTemporal(&f);
    std::printf("refused: returned\n");
  } catch (const std::runtime_error &) {
    std::printf("refused: threw\n");
  }
  return 0;
}
