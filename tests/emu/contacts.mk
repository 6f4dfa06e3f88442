# TEST INFRASTRUCTURE: host builds of the contact record (jaco_set_contact_record) against the wavefront emulator, in the three layouts
# of the library.  Built on demand by tests/test_contacts_emu.py (make -f contacts.mk); flags and layouts come from the Makefile.
include Makefile
CDEPS = emu_contacts.cpp emu_driver.cpp wave_emu.cpp $(CSRC)/model_blob.cpp $(CSRC)/physics_kernel.h $(CSRC)/include/jaco/model_dev.h jaco/wave_ops.h hip/hip_runtime.h ../../include/jaco_env.h $(wildcard $(CSRC)/*.h)
CSRCS = emu_contacts.cpp wave_emu.cpp $(CSRC)/model_blob.cpp
.DEFAULT_GOAL := contacts
contacts: libjaco_emu_contacts.so libjaco_emu_contacts_d12.so libjaco_emu_contacts_d30.so
libjaco_emu_contacts.so: $(CDEPS)
	$(CXX) $(CXXFLAGS) -shared -o $@ $(CSRCS)
libjaco_emu_contacts_d12.so: $(CDEPS)
	$(CXX) $(CXXFLAGS) $(D12) -shared -o $@ $(CSRCS)
libjaco_emu_contacts_d30.so: $(CDEPS)
	$(CXX) $(CXXFLAGS) $(D30) -shared -o $@ $(CSRCS)
# the A/B build options of the kernel with the record on (built on demand, not part of `contacts`)
libjaco_emu_contacts_wrench.so: $(CDEPS)
	$(CXX) $(CXXFLAGS) -DJACO_WRENCH=1 -shared -o $@ $(CSRCS)
libjaco_emu_contacts_nolook.so: $(CDEPS)
	$(CXX) $(CXXFLAGS) -DJACO_NEWTON_LOOKAHEAD=0 -shared -o $@ $(CSRCS)
libjaco_emu_contacts_mprpairs.so: $(CDEPS)
	$(CXX) $(CXXFLAGS) -DJACO_MPR_PAIRS=1 -shared -o $@ $(CSRCS)
