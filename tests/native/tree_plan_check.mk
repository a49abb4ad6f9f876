# Host build of tree_plan_check (test infrastructure, never linked into the library): the one-launch tree search's LDS plans, their
# ladder, the flattened trajectory lists and the alignment record of mg_tree_plan.h against a restatement (see tree_plan_check.cpp).
# A program of its own, under the address and undefined-behaviour sanitizers where the compiler has their runtimes, plain where it
# has not, with the library's floating-point contract (every fma spelled out).  tests/test_cluster_tree_trajectories_host.py runs
#     make -C tests/native -f tree_plan_check.mk
CSRC = ../../morphablegraphs_amd/csrc
FLAGS = -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fno-fast-math

tree_plan_check: tree_plan_check.cpp $(CSRC)/mg_tree_plan.h $(CSRC)/mg_hostdefs.h ../../include/mg_hip.h
	$(CXX) $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ tree_plan_check.cpp 2>/dev/null || $(CXX) $(FLAGS) -o $@ tree_plan_check.cpp
