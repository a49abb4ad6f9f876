# Host build of savgol_table_check (test infrastructure, never linked into the library): the 225 doubles of mg_savgol_table.h, printed
# as hex for the comparison with time_smoothing.savgol_hat_matrix(), and the table's own properties (see savgol_table_check.cpp).
# A program of its own, under the address and undefined-behaviour sanitizers where the compiler has their runtimes, plain where it
# has not, with the library's floating-point contract.  tests/test_time_smoothing_host.py runs
#     make -C tests/native -f savgol_table_check.mk
CSRC = ../../morphablegraphs_amd/csrc
FLAGS = -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fno-fast-math

savgol_table_check: savgol_table_check.cpp $(CSRC)/mg_savgol_table.h
	@if $(CXX) $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ savgol_table_check.cpp 2>$@.log; \
	then echo "savgol_table_check: built with the address and undefined-behaviour sanitizers"; rm -f $@.log; \
	else echo "savgol_table_check: the sanitized build failed (see below); building plain"; cat $@.log; rm -f $@.log; $(CXX) $(FLAGS) -o $@ savgol_table_check.cpp; fi
