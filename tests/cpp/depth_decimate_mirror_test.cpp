// depth_decimate_mirror_test.cpp — SceneFlowConstructor::setDepthDecimation exists and forwards to mod_set_depth_decimation, without
// the library: mirror_calls_test.cpp's call recorder stands in for it (its ModContext, its stubs and its Rig; its main is renamed and
// not run), and the one stub it lacks is defined here.  tests/test_depth_decimate_abi.py reads the lines that begin with the call's name.
#define main mirror_calls_main
#include "mirror_calls_test.cpp"
#undef main

int mod_set_depth_decimation(ModContext *c, const ModDepthDecimation *d) {
  if (d) std::printf("mod_set_depth_decimation %d %d %d %d %g %g %d %d\n", d->dx, d->dy, d->mode, d->min_valid, d->tol_abs, d->tol_rel, d->reserved[0], d->reserved[1]);
  else std::printf("mod_set_depth_decimation NULL\n");
  return c->code("mod_set_depth_decimation");
}

int main() {
  Rig r;
  const ModDepthDecimation d{2, 3, MOD_DEPTH_DECIMATE_MEAN, 4, 0.25f, 0.125f, {0, 0}};
  r.sfc.setDepthDecimation(&d);
  r.sfc.setDepthDecimation(nullptr);
  r.ctx.codes["mod_set_depth_decimation"] = {MOD_ERR_INVALID_ARGUMENT};     // a refusal becomes an exception, like every setter's
  try {
    r.sfc.setDepthDecimation(&d);
    std::printf("refused: returned\n");
  } catch (const std::runtime_error &) {
    std::printf("refused: threw\n");
  }
  return 0;
}
