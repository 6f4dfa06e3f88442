# TEST INFRASTRUCTURE: host builds of the robot-configuration query kernel (emu_query.cpp) against the wavefront emulator, in the three
# layouts of the library.  Built on demand by tests/test_query_emu.py (make -f query.mk); flags and layouts come from the Makefile.
include Makefile
QDEPS = emu_query.cpp emu_driver.cpp wave_emu.cpp $(CSRC)/model_blob.cpp $(CSRC)/physics_kernel.h $(CSRC)/include/jaco/model_dev.h jaco/wave_ops.h hip/hip_runtime.h ../../include/jaco_env.h $(wildcard $(CSRC)/*.h)
QSRC = emu_query.cpp emu_driver.cpp wave_emu.cpp $(CSRC)/model_blob.cpp
.DEFAULT_GOAL := query
query: libjaco_emu_query.so libjaco_emu_query_d12.so libjaco_emu_query_d30.so
libjaco_emu_query.so: $(QDEPS)
	$(CXX) $(CXXFLAGS) -shared -o $@ $(QSRC)
libjaco_emu_query_d12.so: $(QDEPS)
	$(CXX) $(CXXFLAGS) $(D12) -shared -o $@ $(QSRC)
libjaco_emu_query_d30.so: $(QDEPS)
	$(CXX) $(CXXFLAGS) $(D30) -shared -o $@ $(QSRC)
