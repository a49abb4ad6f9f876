# Host build of tree_frames_plan_check (test infrastructure, never linked into the library): the per-frame lists' LDS regions, the
# further rungs of the one-launch tree search's ladder and the slab's size of mg_tree_plan.h against a restatement (see
# tree_frames_plan_check.cpp).  A program of its own, under the address and undefined-behaviour sanitizers where the compiler has their
# runtimes, plain where it has not.  tests/test_tree_search_frames_host.py runs
#     make -C tests/native -f tree_frames_plan_check.mk
CSRC = ../../morphablegraphs_amd/csrc
FLAGS = -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fno-fast-math

tree_frames_plan_check: tree_frames_plan_check.cpp $(CSRC)/mg_tree_plan.h $(CSRC)/mg_hostdefs.h ../../include/mg_hip.h
	$(CXX) $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ tree_frames_plan_check.cpp 2>/dev/null || $(CXX) $(FLAGS) -o $@ tree_frames_plan_check.cpp
