# launch_pcm_requantize on its own (alac_amd/csrc/alac_pcm_in.hip compiled into the program, host side sanitized) — tests/test_launch_status_int.py
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := $(ROOT)/alac_amd/csrc
launch_status_int: launch_status_int.hip $(CSRC)/alac_pcm_in.hip $(wildcard $(CSRC)/*.hpp)
	$(HIPCC) -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Wall -Wno-unused-function -I$(CSRC) -I$(ROOT)/include launch_status_int.hip $(CSRC)/alac_pcm_in.hip -o $@
