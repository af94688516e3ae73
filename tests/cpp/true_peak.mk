# harness of ALACDecoder::LoudnessTruePeakBatch (tests/test_gpu_alacconvert_true_peak.py): make -C tests/cpp -f true_peak.mk
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
HIPCC ?= /opt/rocm/bin/hipcc
true_peak: true_peak.cpp $(ROOT)/alac_amd/libalac_hip.so $(ROOT)/include/alac/ALACDecoder.h $(ROOT)/include/alac_hip.h
	$(HIPCC) -O2 -std=c++17 -I$(ROOT)/include/alac -I$(ROOT)/include $< -o $@ -L$(ROOT)/alac_amd -lalac_hip -Wl,-rpath,'$$ORIGIN/../../alac_amd'
