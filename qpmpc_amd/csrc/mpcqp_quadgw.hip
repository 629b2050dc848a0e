// mpcqp_quadgw.hip -- the general four-per-wavefront kernel with four rows per lane (csrc/mpcqp_quadg.hip: 33 .. 64 rows at n <= 16),
// instantiated for the streamed build of nx = 5 .. 8, compiled as a unit of its own for the build time. Same source, same reference
// code (qpmpc/mpc_qp.py:53-149, qpmpc/solve_mpc.py:43).
#define MPCQP_QUADG_WIDE_UNIT 1
#include "mpcqp_quadg.hip"
