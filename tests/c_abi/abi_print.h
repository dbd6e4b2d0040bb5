/* abi_print.h -- how the *_abi_check.c programs print a layout as the C compiler sees it, one line per fact, for
 * tests/abi_support.py::c_layouts to compare with the ctypes structures:
 *     sizeof <which> <bytes>
 *     <which>.<field> <offset>
 * Plain C99: the programs are built with -pedantic -Werror. */
#ifndef CAVMD_TESTS_ABI_PRINT_H_
#define CAVMD_TESTS_ABI_PRINT_H_

#include <stddef.h>
#include <stdio.h>

#define ABI_SIZE(which, type) printf("sizeof " #which " %u\n", (unsigned)sizeof(type))
#define ABI_OFF(which, type, field) printf(#which "." #field " %u\n", (unsigned)offsetof(type, field))

#endif
