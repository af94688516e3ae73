# harness of ALACEncoder::EncodeSegmentsInt and the integer host forms (tests/test_gpu_encode_int.py):
# make -C tests/cpp -f encode_int.mk
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
HIPCC ?= /opt/rocm/bin/hipcc
encode_int: encode_int.cpp $(ROOT)/alac_amd/libalac_hip.so $(ROOT)/include/alac/ALACEncoder.h $(ROOT)/include/alac_hip.h
	$(HIPCC) -O2 -std=c++17 -I$(ROOT)/include/alac -I$(ROOT)/include $< -o $@ -L$(ROOT)/alac_amd -lalac_hip -Wl,-rpath,'$$ORIGIN/../../alac_amd'
