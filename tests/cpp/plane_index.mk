# the index rule of the encoder's residual planes (alac_amd/csrc/alac_plane_index.hpp, host build) on its own, sanitized
# (tests/test_plane_index.py)
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
plane_index: plane_index.cpp $(ROOT)/alac_amd/csrc/alac_plane_index.hpp
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra -I$(ROOT)/alac_amd/csrc $< -o $@
