// TEST INFRASTRUCTURE: the contact record (jaco_set_contact_record, include/jaco_env.h) under the lockstep wavefront emulator -- a
// ctrl-level step (emu_driver.cpp's launch sequence: light grid, then the medium / heavy / huge drains) with the record fields of the
// argument block set.  Built by tests/emu/contacts.mk into libjaco_emu_contacts{,_d12,_d30}.so; this unit takes the place of
// emu_driver.cpp, whose every entry point the library keeps.
#include "emu_driver.cpp"
#include "../../include/jaco_env.h"

static_assert(sizeof(JacoContact) == sizeof(JacoContactRec), "JacoContact (include/jaco_env.h) and JacoContactRec (physics_kernel.h) disagree");

extern "C" int emu_contact_words() { return (int)(sizeof(JacoContact) / 4); }

// emu_physics_step with the record: rec [nenv][cap] / ncon [nenv], or rec = NULL (off; what jaco_set_contact_record(h, NULL, ...) leaves)
extern "C" int emu_contacts_step(const void* blob, long blob_size, int nenv, int nsub, int disable_contact, float* qpos, float* qvel, float* qacc_ws,
                                 const float* ctrl, float* sensordata, unsigned* flags, int* stats, JacoContact* rec, int* ncon, int cap, int* heavy_envs) {
  if (rec && (!ncon || cap < 1 || cap > JACO_CONTACT_MAX_CAPACITY)) return JACO_EINVAL;
  std::string err;
  if (jaco_model_from_blob(blob, (size_t)blob_size, &g_model, &g_hull, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return -1; }
  if (g_mpr_output >= 0) g_model.mpr_output = g_mpr_output;
  JacoStepArgs A{};
  A.model = &g_model; A.hull = g_hull.data(); A.qpos = qpos; A.qvel = qvel; A.qacc_ws = qacc_ws; A.ctrl = ctrl; A.sensordata = sensordata;
  A.flags = flags; A.stats = stats; A.nenv = nenv; A.nsub = nsub; A.disable_contact = disable_contact; A.dbg_env = -1;
  A.con_rec = rec ? reinterpret_cast<JacoContactRec*>(rec) : nullptr; A.con_n = rec ? ncon : nullptr; A.con_cap = rec ? cap : 0;
  return emu_launch(A, heavy_envs);
}
