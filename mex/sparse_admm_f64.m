function [S, convergence_error] = sparse_admm_f64(Htrue, OH, Dr, Dt, Imax)
% benchmark_algorithms/sparse_admm.m evaluated in float64 on the MI355X (jstsp_sparse_admm_f64): Grams, eigen-decompositions,
% products and the error curve in double - nothing is narrowed.  Same signature as sparse_admm.m; pages of OH = batch.
  [S, convergence_error] = jstsp_mex('sparse_admm_f64', Htrue, OH, Dr, Dt, Imax);
end
