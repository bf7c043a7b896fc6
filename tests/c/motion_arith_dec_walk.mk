# The arithmetic motion-data decoder's host code under ASan + UBSan (tests/test_motion_arith_dec_host_sanitized.py): motion_arith_dec_walk.cpp, a plain C++
# program with its own main, compiled host-only with the sanitizer and linked with the OBJECTS of the device-free
# sanitizer build of the library (make -C schroedinger_amd/csrc dry_asan leaves them in dry_asan/) -- one image, the
# sanitizer's runtime linked into the program itself, nothing preloaded.  Needs no device; -fno-gpu-sanitize says outright
# that the sanitizer is for the host code alone.
#   make -f motion_arith_dec_walk.mk motion_arith_dec_walk_asan
ROOT = ../..
CSRC = $(ROOT)/schroedinger_amd/csrc
LIBDIR = $(ROOT)/schroedinger_amd
HIPCC ?= /opt/rocm/bin/hipcc
WALKFLAGS = -O1 -g -fno-omit-frame-pointer -std=c++17 -Wall -I$(ROOT)/include

motion_arith_dec_walk_asan: _build/motion_arith_dec_walk_asan

# (the library's own Makefile decides whether its objects are up to date)
$(LIBDIR)/libschro_hip_dry_asan.so: FORCE
	$(MAKE) -C $(CSRC) dry_asan
FORCE:

_build/motion_arith_dec_walk_asan: motion_arith_dec_walk.cpp $(ROOT)/include/schro_hip.h $(LIBDIR)/libschro_hip_dry_asan.so
	mkdir -p _build
	$(HIPCC) --offload-host-only -x c++ $(WALKFLAGS) -fsanitize=address,undefined -fno-gpu-sanitize -fno-sanitize=vptr,function -c motion_arith_dec_walk.cpp -o _build/motion_arith_dec_walk_asan.o
	$(HIPCC) -fsanitize=address,undefined -fno-gpu-sanitize _build/motion_arith_dec_walk_asan.o $(CSRC)/dry_asan/*.o -lpthread -o $@

.PHONY: motion_arith_dec_walk_asan FORCE
