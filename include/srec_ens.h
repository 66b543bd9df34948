/* The host descriptor of the multi-table served score (csrc/ensemble.hip): srec_served_multi, what `const void* desc` of
 * srec_ens_select / srec_ens_ahead points to.  include/srec.h includes this file and states the contract (section "serving
 * and evaluation of ENSEMBLES"); the Python side binds the struct and SREC_ENS_MAXCOMP from THIS file (_lib.ENS_STRUCTS /
 * _lib.ENS_CONST, laid out by _lib.parse_structs like the structs of srec.h and srec_hg.h): to extend the struct, edit this
 * header only.  A HOST struct of DEVICE pointers, read during the call only.  Entries >= C of the arrays are not read. */
#ifndef SREC_ENS_H
#define SREC_ENS_H

#define SREC_ENS_MAXCOMP 8
typedef struct srec_served_multi {
    const float* sr[SREC_ENS_MAXCOMP]; int ld_sr[SREC_ENS_MAXCOMP];   /* the session vectors of every component */
    const float* E[SREC_ENS_MAXCOMP]; int ld_e[SREC_ENS_MAXCOMP];     /* its table */
    const float* cs[SREC_ENS_MAXCOMP];                                /* its column scale */
    int d[SREC_ENS_MAXCOMP];                                          /* its width */
    int C;
    const float* off_ex; const float* off_in;
    const int* listed; int L; int listed_mode;
    long id_lo;
    int B, V;
    const float* bias; long ld_bias;
    const int* group; int G;
} srec_served_multi;

#endif
