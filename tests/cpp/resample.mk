# harness of alac_hip_resample_int_host / alac_hip_resample_float_host (tests/test_gpu_resample_host.py): make -C tests/cpp -f resample.mk
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
HIPCC ?= /opt/rocm/bin/hipcc
resample: resample.cpp $(ROOT)/alac_amd/libalac_hip.so $(ROOT)/include/alac_hip.h
	$(HIPCC) -O2 -std=c++17 -I$(ROOT)/include $< -o $@ -L$(ROOT)/alac_amd -lalac_hip -Wl,-rpath,'$$ORIGIN/../../alac_amd'
