/*
 * oracle/ref_shim/mpi/mpi.h -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference driver main.c includes <mpi.h>.  `make ref` compiles that driver against include/smatcher.h into
 * _ref/main.o (never linked) so that tests/test_host.py can read which library symbols it needs; these declarations
 * of the MPI calls it makes are all the translation unit has to see.
 */
#ifndef ORACLE_REF_SHIM_MPI_H
#define ORACLE_REF_SHIM_MPI_H
typedef int MPI_Comm; typedef int MPI_Datatype; typedef int MPI_Op;
#define MPI_COMM_WORLD 0
#define MPI_CHAR 1
#define MPI_INT 2
#define MPI_DOUBLE 3
#define MPI_SUM 4
#define MPI_UNSIGNED_CHAR 5
int MPI_Init(int*, char***); int MPI_Comm_size(MPI_Comm, int*); int MPI_Comm_rank(MPI_Comm, int*); int MPI_Barrier(MPI_Comm);
double MPI_Wtime(void); int MPI_Finalize(void);
int MPI_Scatterv(const void*, const int*, const int*, MPI_Datatype, void*, int, MPI_Datatype, int, MPI_Comm);
int MPI_Bcast(void*, int, MPI_Datatype, int, MPI_Comm);
int MPI_Reduce(const void*, void*, int, MPI_Datatype, MPI_Op, int, MPI_Comm);
#endif
