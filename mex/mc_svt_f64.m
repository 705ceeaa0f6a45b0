function X = mc_svt_f64(OH, Omega, Imax, tau, rho)
% X = mc_svt(OH, Omega, Imax, tau, rho) (benchmark_algorithms/mc_svt.m) in float64 on the MI355X (jstsp_mc_svt_f64):
% the singular-value threshold runs to convergence in every iteration and nothing is narrowed.  The pages of OH are
% independent problems; tau and rho are scalars or one value per page.
  X = jstsp_mex('mc_svt_f64', OH, Omega, Imax, tau, rho);
end
