function [X, convergence_error] = mc_admm_f64(Htrue, OH, Omega, Imax, tau, rho)
% [X, convergence_error] = mc_admm(Htrue, OH, Omega, Imax, tau, rho) (benchmark_algorithms/mc_admm.m) in float64 on the
% MI355X (jstsp_mc_admm_f64).  The pages of OH are independent problems.  With one output the error curve is not
% computed and Htrue may be [].
  if nargout >= 2
    [X, convergence_error] = jstsp_mex('mc_admm_f64', Htrue, OH, Omega, Imax, tau, rho);
  else
    X = jstsp_mex('mc_admm_f64', Htrue, OH, Omega, Imax, tau, rho);
  end
end
