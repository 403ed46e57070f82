// Intentionally empty: not compiled (the Makefile's SRCS does not list it).
//
// This file held the 32x32x32 MFMA kernels of round 1, a second implementation of layers 1 - 6 that later lived in the
// alternate build only.  Library 0.3.x removed them; `git log -- <this file>` finds the last version.
// The name stays because bench.py fingerprints the kernel sources by file name (KERNEL_SOURCES) to match a PMC summary
// to the sources it was measured on.
