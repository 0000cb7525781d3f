# GuSTOHIPBatch.jl -- include after GuSTOHIP.jl: the entry points that have no counterpart with the same signature in the
# reference -- indirect shooting on the GPU for solve_SCPshooting! and the batched / multi-GPU solve.

# solve!(SS, SP) on the GPU (src/shooting.jl:4-49; DubinsCar and AstrobeeSE3Manifold): the handle that holds the SCP state of SP's problem runs the
# batched indirect shooting from SP.p0 (= SCPS.dual).  Use it in place of `solve!` inside solve_SCPshooting!
# (src/traj_opt.jl:28): `ss_sol = solve_shooting_hip!(SS, SP, SCPS)`.
struct GustoShootOpts      # gusto_shoot_opts
  substeps::Cint; max_newton::Cint; ftol::Cdouble; no_group_pass::Cint
end
function solve_shooting_hip!(SS::ShootingSolution, SP::ShootingProblem, SCPS::SCPSolution; substeps=4, max_newton=100, ftol=1e-3)
  h = get(GUSTO_HANDLES, SCPS, C_NULL)
  h == C_NULL && error("solve_shooting_hip!: run solve_gusto_hip! on this SCPSolution first")
  model, N = SP.PD.model, SP.N
  n, m = model.x_dim, model.u_dim
  t0 = time_ns()
  gusto_check(ccall((:gusto_shoot, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{GustoShootOpts}),
                    h, Float64.(SP.p0), GustoShootOpts(substeps, max_newton, ftol, 0)), h, "shoot")
  st, it, res, p0 = zeros(Cint, 1), zeros(Cint, 1), zeros(1), zeros(n)
  X, U = zeros(n, N), zeros(m, N)
  gusto_check(ccall((:gusto_get_shoot, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), h, st, it, res, p0, X, U), h, "get_shoot")
  el = (time_ns() - t0) / 10^9
  if st[1] == 1                                   # sol_newton.f_converged
    new_traj = Trajectory(X, U, SP.tf)
    push!(SS.prob_status, :Optimal); push!(SS.J_true, cost_true(new_traj, new_traj, SP))
    push!(SS.convergence_measure, convergence_metric(new_traj, SS.traj, SP)); copy!(SS.traj, new_traj)
  else
    push!(SS.prob_status, :Diverged); push!(SS.J_true, NaN); push!(SS.convergence_measure, NaN)
  end
  push!(SS.iter_elapsed_times, el)
  nothing
end

# Batch entry point (the reference has none): every TOP must share model and N (each may bring its own environment).  `devices` = GPU ordinals:
# the problems are split in contiguous blocks of ceil(B/G) (SURVEY.md 8(e)), one handle per entry, every block enqueued
# with gusto_solve_async so the GPUs run concurrently; the results come back in problem order.
# gusto_set_decomposition (include/gusto_hip.h): how a solve maps problems to the GPU.  AUTO picks by batch size -- for astrobeeSE3 /
# astrobeeSE3manifold two or four wavefronts per problem (a wave per Riccati chain of the horizon) while the batch leaves SIMDs idle.
const GUSTO_DECOMP_AUTO, GUSTO_DECOMP_WAVE, GUSTO_DECOMP_LANE, GUSTO_DECOMP_WAVE2, GUSTO_DECOMP_WAVE4 = Cint(0), Cint(1), Cint(2), Cint(3), Cint(4)   # (LANE: reserved, refused)

function solve_SCP_batch!(TOSs::Vector, TOPs::Vector, init_method=init_traj_straightline; max_iter=30, force=false, device=0, devices=nothing,
                          decomposition=GUSTO_DECOMP_AUTO)
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, B = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N, TOPs) ||
    error("solve_SCP_batch!: all problems must share the model type and N")
  # every ProblemDefinition owns its env (types.jl:32-39): problems with different environments go through
  # gusto_set_env_batch (one Workspace per problem), a batch sharing one env through gusto_set_env
  same_env = all(T -> T.PD.env === TOP0.PD.env, TOPs)
  envs = same_env ? nothing : [gusto_env_tables(T.PD.env) for T in TOPs]
  devs = devices === nothing ? [device] : collect(devices)
  G = length(devs); per = cld(B, G)
  boxes, spheres = gusto_env_tables(TOP0.PD.env)
  alg0 = SCPParam_GuSTO(model)
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail,
                      SCPParam(model, TOP0.fixed_final_time).convergence_threshold)
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat(first.(bounds)...), hcat(last.(bounds)...)
  tf = Float64[T.tf_guess for T in TOPs]
  inits = [init_method(T) for T in TOPs]
  X0, U0 = cat((t.X for t in inits)..., dims=3), cat((t.U for t in inits)..., dims=3)   # [n,N,B]: problem slowest
  shards = Tuple{Int,Int,Ptr{Cvoid}}[]
  for (r, dv) in enumerate(devs)
    b0, b1 = min(B, (r - 1) * per) + 1, min(B, r * per)
    b1 < b0 && continue
    href = Ref{Ptr{Cvoid}}(C_NULL)
    gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                      href, gusto_model_id(model), N, b1 - b0 + 1, gusto_hist_cap(max_iter), dv), href[], "create")
    h = href[]
    decomposition == GUSTO_DECOMP_AUTO ||
      gusto_check(ccall((:gusto_set_decomposition, libgusto_hip), Cint, (Ptr{Cvoid}, Cint), h, decomposition), h, "set_decomposition")
    gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                      h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
    gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                      h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
    if !same_env
      nb = Cint[length(e[1]) ÷ 6 for e in envs[b0:b1]]; ns = Cint[length(e[2]) ÷ 4 for e in envs[b0:b1]]
      bx = vcat((vec(e[1]) for e in envs[b0:b1])...); sx = vcat((vec(e[2]) for e in envs[b0:b1])...)
      gusto_check(ccall((:gusto_set_env_batch, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}),
                        h, b1 - b0 + 1, nb, bx, ns, sx), h, "set_env_batch")
    end
    gusto_check(ccall((:gusto_set_problems, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                      h, b1 - b0 + 1, x0[:, b0:b1], lo[:, b0:b1], hi[:, b0:b1], tf[b0:b1], X0[:, :, b0:b1], U0[:, :, b0:b1]), h, "set_problems")
    gusto_check(ccall((:gusto_solve_async, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, max_iter, force), h, "solve_async")
    push!(shards, (b0, b1, h))
  end
  # the final gather of the multi-GPU path (north_star: "RCCL over xGMI for the final gather"; one process here, so direct
  # peer copies): every shard to the first handle's GPU, one hop each over xGMI, then ONE copy to the host
  Xall, Uall = zeros(n, N, B), zeros(m, N, B)
  if length(shards) > 1
    hs = Ptr{Cvoid}[h for (_, _, h) in shards]
    gusto_check(ccall((:gusto_gather_peer, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cdouble}}, Ptr{Ptr{Cdouble}}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                      hs[1], length(hs), hs, C_NULL, C_NULL, Xall, Uall, C_NULL), hs[1], "gather_peer")
  end
  for (b0, b1, h) in shards
    Bs = b1 - b0 + 1
    gusto_check(ccall((:gusto_wait, libgusto_hip), Cint, (Ptr{Cvoid},), h), h, "wait")
    X, U = zeros(n, N, Bs), zeros(m, N, Bs)
    if length(shards) > 1
      X .= Xall[:, :, b0:b1]; U .= Uall[:, :, b0:b1]
    else
      gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
    end
    its, conv, succ, stop = zeros(Cint, Bs), zeros(Cint, Bs), zeros(Cint, Bs), zeros(Cint, Bs)
    gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}),
                      h, its, conv, succ, stop, C_NULL), h, "get_status")
    duals = zeros(n, Bs)
    gusto_check(ccall((:gusto_get_dual, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, duals), h, "get_dual")
    Hs = gusto_histories(h, Bs)                      # one device -> host copy per shard
    msec = Ref{Cdouble}(0.)
    ccall((:gusto_last_solve_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, msec)
    for b in b0:b1
      j = b - b0 + 1
      SCPP = SCPProblem(TOPs[b])
      SCPP.param.alg = SCPParam_GuSTO(model)
      SCPS = SCPSolution(SCPP, Trajectory(X[:, :, j], U[:, :, j], TOPs[b].tf_guess))
      gusto_fill_solution!(SCPS, SCPP.param.alg, Hs, j, its[j], conv[j], succ[j], stop[j], duals[:, j])
      SCPS.total_time = msec[] / 1e3 / Bs
      SCPS.iter_elapsed_times = vcat(0., fill(SCPS.total_time / max(1, its[j]), its[j]))
      SCPP.param.obstacle_toggle_distance = SCPP.param.alg.Δ_vec[end] / 8 + model.clearance
      TOSs[b].traj, TOSs[b].SCPS = SCPS.traj, SCPS
    end
    ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  end
  nothing
end

# ---- TrajOpt behind the same seam: solve_SCP!(TOS, TOP, solve_trajopt_hip!, init_traj_straightline, "hip") -----------------
# positional signature of solve_trajopt_jump! (src/scp/scp_trajopt.jl:33); FreeflyerSE2 and AstrobeeSE3
struct GustoTrajOptParams      # gusto_trajopt_params
  mu0::Cdouble; s0::Cdouble; c::Cdouble; tau_plus::Cdouble; tau_minus::Cdouble; k::Cdouble; ftol::Cdouble; xtol::Cdouble; ctol::Cdouble
  max_penalty_iteration::Cint; max_convex_iteration::Cint; max_trust_iteration::Cint
end

mutable struct GustoTrajOptHistory  # gusto_trajopt_history
  hist_cap::Cint
  n_solves::Ptr{Cint}; n_mu::Ptr{Cint}; n_xtol::Ptr{Cint}; n_ftol::Ptr{Cint}; n_ctol::Ptr{Cint}
  rho_vec::Ptr{Cdouble}; s_vec::Ptr{Cdouble}; mu_vec::Ptr{Cdouble}; xtol_vec::Ptr{Cdouble}; ftol_vec::Ptr{Cdouble}; ctol_vec::Ptr{Cdouble}
  J_true::Ptr{Cdouble}; J_full::Ptr{Cdouble}; convergence_measure::Ptr{Cdouble}
  solver_status::Ptr{Cint}; ipm_iters::Ptr{Cint}
end

function solve_trajopt_hip!(SCPS::SCPSolution, SCPP::SCPProblem, solver="hip", max_iter=125, force=false; device=0, kwarg...)
  model, N = SCPP.PD.model, SCPP.N
  n, m = model.x_dim, model.u_dim
  SCPP.param.alg = SCPParam_TrajOpt(model)                       # :44
  a = SCPP.param.alg
  tp = GustoTrajOptParams(a.mu0, a.s0, a.c, a.τ_plus, a.τ_minus, a.k, a.ftol, a.xtol, a.ctol,
                          a.max_penalty_iteration, a.max_convex_iteration, a.max_trust_iteration)
  cap = 2 * a.max_penalty_iteration * a.max_convex_iteration * a.max_trust_iteration + 16
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create_trajopt, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, 1, cap, device), href[], "create_trajopt")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{GustoModelParams}),
                    h, C_NULL, gusto_model_params(SCPP.PD.robot, model)), h, "set_params")
  gusto_check(ccall((:gusto_set_trajopt_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoTrajOptParams}), h, tp), h, "set_trajopt_params")
  boxes, spheres = gusto_env_tables(SCPP.PD.env)
  gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                    h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
  lo, hi = gusto_goal_bounds(SCPP.PD.goal_set, n, SCPP.tf_guess)
  gusto_check(ccall((:gusto_set_problems, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    h, 1, Float64.(SCPP.PD.x_init), lo, hi, [Float64(SCPP.tf_guess)], Matrix{Float64}(SCPS.traj.X), Matrix{Float64}(SCPS.traj.U)), h, "set_problems")
  t0 = time_ns()
  gusto_check(ccall((:gusto_solve_trajopt, libgusto_hip), Cint, (Ptr{Cvoid}, Cint), h, max_iter), h, "solve_trajopt")
  elapsed = (time_ns() - t0) / 10^9
  X, U = zeros(n, N), zeros(m, N)
  gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
  SCPS.traj.X, SCPS.traj.U = X, U
  its, conv, stop = zeros(Cint, 1), zeros(Cint, 1), zeros(Cint, 1)
  gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}, Ptr{Cint}, Ptr{Cvoid}),
                    h, its, conv, C_NULL, stop, C_NULL), h, "get_status")
  d() = zeros(Cdouble, cap); ns, nm, nx, nf, nc = (zeros(Cint, 1) for _ in 1:5)
  rho, sv, muv, xt, ft, ct, Jt, Jf, cm = (d() for _ in 1:9)
  sol, ipi = zeros(Cint, cap), zeros(Cint, cap)
  hist = GustoTrajOptHistory(cap, pointer(ns), pointer(nm), pointer(nx), pointer(nf), pointer(nc), pointer(rho), pointer(sv), pointer(muv),
                             pointer(xt), pointer(ft), pointer(ct), pointer(Jt), pointer(Jf), pointer(cm), pointer(sol), pointer(ipi))
  GC.@preserve ns nm nx nf nc rho sv muv xt ft ct Jt Jf cm sol ipi begin
    gusto_check(ccall((:gusto_get_trajopt_history, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoTrajOptHistory}), h, hist), h, "get_trajopt_history")
  end
  S = Int(ns[1])
  SCPS.J_true, SCPS.J_full = Jt[1:S+1], Jf[1:S]
  SCPS.convergence_measure = vcat(0., cm[2:S+1])
  SCPS.solver_status = [GUSTO_SOLVER_STATUS[s+1] for s in sol[1:S+1]]
  SCPS.iterations, SCPS.converged = S, conv[1] != 0
  SCPS.total_time += elapsed
  SCPS.iter_elapsed_times = vcat(0., fill(SCPS.total_time / max(1, S), S))
  dual = zeros(n)
  gusto_check(ccall((:gusto_get_dual, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, dual), h, "get_dual")
  SCPS.dual = dual
  a.ρ_vec, a.s_vec, a.mu_vec = rho[1:S+1], sv[1:S+1], muv[1:nm[1]]
  a.xtol_vec, a.ftol_vec, a.ctol_vec = xt[1:nx[1]], ft[1:nf[1]], ct[1:nc[1]]
  SCPP.param.obstacle_toggle_distance = model.clearance + 1.     # :64
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  nothing
end

# ---- solve_SCPshooting! (src/traj_opt.jl:4-45) for a batch on ONE handle ---------------------------------------------------
# Per round one gusto_shoot and one gusto_solve(h, 1, 0) over the problems still in their loop; gusto_set_active carries the
# per-problem loop condition `!SCPS.converged && SCPS.iterations < max_iter` (traj_opt.jl:23).  Mirrors
# gusto.jl_amd/host.py: solve_SCPshooting_batch (which the GPU tests hold bit for bit against the single-problem driver).
function solve_SCPshooting_batch!(TOSs::Vector, TOPs::Vector, init_method=init_traj_straightline; max_iter=30, device=0)
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, B = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N, TOPs) ||
    error("solve_SCPshooting_batch!: all problems must share the model type and N")
  # ONE handle = one set of SCP and model parameters: a batch of different robots or thresholds is refused, not solved with problem 1's
  mp0 = gusto_model_params(TOP0.PD.robot, model)
  all(T -> isequal(gusto_model_params(T.PD.robot, T.PD.model), mp0) && T.fixed_final_time == TOP0.fixed_final_time, TOPs) ||
    error("solve_SCPshooting_batch!: all problems must share the model / robot parameters and the SCP parameters")
  alg0 = SCPParam_GuSTO(model)
  thr = SCPParam(model, TOP0.fixed_final_time).convergence_threshold
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail, thr)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, B, gusto_hist_cap(max_iter), device), href[], "create")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                    h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
  envs = [gusto_env_tables(T.PD.env) for T in TOPs]
  nb = Cint[length(e[1]) ÷ 6 for e in envs]; ns = Cint[length(e[2]) ÷ 4 for e in envs]
  gusto_check(ccall((:gusto_set_env_batch, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}),
                    h, B, nb, vcat((vec(e[1]) for e in envs)...), ns, vcat((vec(e[2]) for e in envs)...)), h, "set_env_batch")
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat(first.(bounds)...), hcat(last.(bounds)...)
  inits = [init_method(T) for T in TOPs]
  X0, U0 = cat((t.X for t in inits)..., dims=3), cat((t.U for t in inits)..., dims=3)
  gusto_check(ccall((:gusto_set_problems, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    h, B, x0, lo, hi, Float64[T.tf_guess for T in TOPs], X0, U0), h, "set_problems")
  SCPPs = [SCPProblem(T) for T in TOPs]
  for P in SCPPs; P.param.alg = SCPParam_GuSTO(model); end
  SCPSs = [SCPSolution(SCPPs[b], inits[b]) for b in 1:B]
  stops = zeros(Cint, B)
  for b in 1:B
    TOSs[b].SCPS = SCPSs[b]
    TOSs[b].SS = ShootingSolution(ShootingProblem(TOPs[b], SCPSs[b]), deepcopy(inits[b]))
  end
  function scp_round!(live)       # solve_method!(SCPS, SCPP, solver, 1) of every live problem: ONE launch
    gusto_check(ccall((:gusto_set_active, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}), h, Cint.(live)), h, "set_active")
    gusto_check(ccall((:gusto_solve, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, 1, 0), h, "solve")
    X, U = zeros(n, N, B), zeros(m, N, B)
    gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
    its, conv, succ = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
    gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}),
                      h, its, conv, succ, stops, C_NULL), h, "get_status")
    duals = zeros(n, B)
    gusto_check(ccall((:gusto_get_dual, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, duals), h, "get_dual")
    Hs = gusto_histories(h, B)
    for b in findall(live)
      SCPSs[b].traj = Trajectory(X[:, :, b], U[:, :, b], TOPs[b].tf_guess)
      gusto_fill_solution!(SCPSs[b], SCPPs[b].param.alg, Hs, b, its[b], conv[b], succ[b], stops[b], duals[:, b])
    end
  end
  live = trues(B)
  scp_round!(live)
  for b in 1:B; push!(TOSs[b].SS.J_true, SCPSs[b].J_true[1]); end
  by_shooting = falses(B)
  while true
    # (stop reasons 2 / 3 / 4 -- failed subproblem, omega > omega_max, history full -- end a problem's loop: solve_method! would
    # return early for ever without counting an iteration, scp_gusto.jl:107-111,163-166)
    live = [!SCPSs[b].converged && SCPSs[b].iterations < max_iter && !(stops[b] in (2, 3, 4)) && !by_shooting[b] for b in 1:B]
    any(live) || break
    gusto_check(ccall((:gusto_set_active, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}), h, Cint.(live)), h, "set_active")
    t0 = time_ns()
    gusto_check(ccall((:gusto_shoot, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{GustoShootOpts}),
                      h, C_NULL, GustoShootOpts(4, 100, 1e-3, 0)), h, "shoot")     # seeds = SCPS.dual of every problem
    st, it, res, p0 = zeros(Cint, B), zeros(Cint, B), zeros(B), zeros(n, B)
    X, U = zeros(n, N, B), zeros(m, N, B)
    gusto_check(ccall((:gusto_get_shoot, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), h, st, it, res, p0, X, U), h, "get_shoot")
    el = (time_ns() - t0) / 10^9 / count(live)
    for b in findall(live)
      SS, SCPS = TOSs[b].SS, SCPSs[b]
      SP = ShootingProblem(TOPs[b], SCPS)
      if st[b] == 1
        new_traj = Trajectory(X[:, :, b], U[:, :, b], SP.tf)
        push!(SS.prob_status, :Optimal); push!(SS.J_true, cost_true(new_traj, new_traj, SP))
        push!(SS.convergence_measure, convergence_metric(new_traj, SS.traj, SP))
        copy!(SS.traj, new_traj)
      else
        push!(SS.prob_status, :Diverged); push!(SS.J_true, NaN); push!(SS.convergence_measure, NaN)
      end
      push!(SS.iter_elapsed_times, el)
      cm = SS.convergence_measure[end-1:end]
      if SCPS.iterations > 2 && !any(isnan, cm) && sum(cm) <= thr      # traj_opt.jl:30
        SS.converged = true; by_shooting[b] = true
      end
    end
    live = live .& .!by_shooting
    any(live) && scp_round!(live)
  end
  for b in 1:B
    copy!(TOSs[b].traj, by_shooting[b] ? TOSs[b].SS.traj : SCPSs[b].traj)
    TOSs[b].total_time = SCPSs[b].total_time + sum(TOSs[b].SS.iter_elapsed_times)
  end
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  nothing
end

# ---- TrajOpt for a batch, one handle per GPU, shards side by side (gusto_solve_trajopt_async + gusto_wait) -----------------
# The batch counterpart of solve_trajopt_hip! (mirrors host.py: solve_SCP_batch(..., solve_trajopt_hip, devices = [...])):
# contiguous shards of ceil(B/G) problems, every shard's ONE launch enqueued before the first is waited for.
function solve_trajopt_batch!(TOSs::Vector, TOPs::Vector, init_method=init_traj_straightline; max_iter=125, device=0, devices=nothing)
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, B = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N, TOPs) ||
    error("solve_trajopt_batch!: all problems must share the model type and N")
  a = SCPParam_TrajOpt(model)
  tp = GustoTrajOptParams(a.mu0, a.s0, a.c, a.τ_plus, a.τ_minus, a.k, a.ftol, a.xtol, a.ctol,
                          a.max_penalty_iteration, a.max_convex_iteration, a.max_trust_iteration)
  cap = 2 * a.max_penalty_iteration * a.max_convex_iteration * a.max_trust_iteration + 16
  devs = devices === nothing ? [device] : collect(devices)
  G = length(devs); per = cld(B, G)
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat(first.(bounds)...), hcat(last.(bounds)...)
  inits = [init_method(T) for T in TOPs]
  X0, U0 = cat((t.X for t in inits)..., dims=3), cat((t.U for t in inits)..., dims=3)
  envs = [gusto_env_tables(T.PD.env) for T in TOPs]
  shards = Tuple{Int,Int,Ptr{Cvoid}}[]
  for (r, dv) in enumerate(devs)
    b0, b1 = min(B, (r - 1) * per) + 1, min(B, r * per)
    b1 < b0 && continue
    href = Ref{Ptr{Cvoid}}(C_NULL)
    gusto_check(ccall((:gusto_create_trajopt, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                      href, gusto_model_id(model), N, b1 - b0 + 1, cap, dv), href[], "create_trajopt")
    h = href[]
    gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{GustoModelParams}),
                      h, C_NULL, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
    gusto_check(ccall((:gusto_set_trajopt_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoTrajOptParams}), h, tp), h, "set_trajopt_params")
    nb = Cint[length(e[1]) ÷ 6 for e in envs[b0:b1]]; ns = Cint[length(e[2]) ÷ 4 for e in envs[b0:b1]]
    gusto_check(ccall((:gusto_set_env_batch, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}),
                      h, b1 - b0 + 1, nb, vcat((vec(e[1]) for e in envs[b0:b1])...), ns, vcat((vec(e[2]) for e in envs[b0:b1])...)), h, "set_env_batch")
    gusto_check(ccall((:gusto_set_problems, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                      h, b1 - b0 + 1, x0[:, b0:b1], lo[:, b0:b1], hi[:, b0:b1], Float64[T.tf_guess for T in TOPs[b0:b1]],
                      X0[:, :, b0:b1], U0[:, :, b0:b1]), h, "set_problems")
    gusto_check(ccall((:gusto_solve_trajopt_async, libgusto_hip), Cint, (Ptr{Cvoid}, Cint), h, max_iter), h, "solve_trajopt_async")
    push!(shards, (b0, b1, h))
  end
  for (b0, b1, h) in shards
    Bs = b1 - b0 + 1
    gusto_check(ccall((:gusto_wait, libgusto_hip), Cint, (Ptr{Cvoid},), h), h, "wait")
    X, U = zeros(n, N, Bs), zeros(m, N, Bs)
    gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
    its, conv = zeros(Cint, Bs), zeros(Cint, Bs)
    gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                      h, its, conv, C_NULL, C_NULL, C_NULL), h, "get_status")
    duals = zeros(n, Bs)
    gusto_check(ccall((:gusto_get_dual, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, duals), h, "get_dual")
    Jt, Jf, cm = zeros(cap, Bs), zeros(cap, Bs), zeros(cap, Bs)      # rows of `cap` entries, problem slowest
    nsol = zeros(Cint, Bs)
    hist = GustoTrajOptHistory(cap, pointer(nsol), C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL,
                               pointer(Jt), pointer(Jf), pointer(cm), C_NULL, C_NULL)
    GC.@preserve nsol Jt Jf cm begin
      gusto_check(ccall((:gusto_get_trajopt_history, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoTrajOptHistory}), h, hist), h, "get_trajopt_history")
    end
    msec = Ref{Cdouble}(0.)
    ccall((:gusto_last_solve_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, msec)
    for b in b0:b1
      j = b - b0 + 1; S = Int(nsol[j])
      SCPP = SCPProblem(TOPs[b]); SCPP.param.alg = SCPParam_TrajOpt(model)
      SCPS = SCPSolution(SCPP, Trajectory(X[:, :, j], U[:, :, j], TOPs[b].tf_guess))
      SCPS.J_true, SCPS.J_full = Jt[1:S+1, j], Jf[1:S, j]
      SCPS.convergence_measure = vcat(0., cm[2:S+1, j])
      SCPS.iterations, SCPS.converged, SCPS.dual = S, conv[j] != 0, duals[:, j]
      SCPS.total_time = msec[] / 1e3 / Bs
      TOSs[b].traj, TOSs[b].SCPS = SCPS.traj, SCPS
    end
    ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  end
  nothing
end

# ---- post-solve verification on the GPU (gusto_verify / gusto_interpolate, csrc/verify.hip) ---------------------------------
# interpolate_traj, dynamics_constraint_satisfaction and verify_collision_free of the Astrobee model files
# (astrobee_se3_manifold.jl:1011-1077) for every problem of a handle, plus the smallest distance over the dense samples and
# the gap between a rolled-out interval and its next knot.  GuSTO handles only (TrajOpt handles answer GUSTO_ERR_ARG).
struct GustoVerifyOpts      # gusto_verify_opts
  dt_min::Cdouble; nstep::Cint; nstep_cap::Cint; dense_collision::Cint
end
mutable struct GustoVerifyReport      # gusto_verify_report
  collision_free::Ptr{Cint}; first_knot::Ptr{Cint}
  first_dist::Ptr{Cdouble}; min_dist_knots::Ptr{Cdouble}; dyn_defect_l1::Ptr{Cdouble}; min_dist_dense::Ptr{Cdouble}
  min_dense_sample::Ptr{Cint}
  max_gap::Ptr{Cdouble}
end

# the report of B problems of handle h as a NamedTuple of vectors; X [n,N,B], U [m,N,B] or nothing = the handle's own trajectories
function verify_batch!(h::Ptr{Cvoid}, B::Integer, X=nothing, U=nothing; dt_min=0.1, nstep=0, nstep_cap=64, dense_collision=true)
  Xp = X === nothing ? Ptr{Cdouble}(C_NULL) : pointer(X); Up = U === nothing ? Ptr{Cdouble}(C_NULL) : pointer(U)
  GC.@preserve X U gusto_check(ccall((:gusto_verify, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GustoVerifyOpts}),
                    h, Xp, Up, GustoVerifyOpts(dt_min, nstep, nstep_cap, dense_collision ? 1 : 0)), h, "verify")
  free, knot, sample = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
  dist, dknots, defect, ddense, gap = zeros(B), zeros(B), zeros(B), zeros(B), zeros(B)
  GC.@preserve free knot sample dist dknots defect ddense gap begin
    rep = GustoVerifyReport(pointer(free), pointer(knot), pointer(dist), pointer(dknots), pointer(defect), pointer(ddense),
                            pointer(sample), pointer(gap))
    gusto_check(ccall((:gusto_get_verify, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoVerifyReport}), h, rep), h, "get_verify")
  end
  (collision_free = free .!= 0, first_knot = Int.(knot), first_dist = dist, min_dist_knots = dknots, dyn_defect_l1 = defect,
   min_dist_dense = ddense, min_dense_sample = Int.(sample), max_gap = gap)
end

# interpolate_traj(traj, SCPP, dt_min) on the handle that solved SCPS (solve_gusto_hip!): the Trajectory at Nstep RK4 samples per interval
function interpolate_traj_hip(traj::Trajectory, SCPS::SCPSolution, dt_min=0.1)
  h = get(GUSTO_HANDLES, SCPS, C_NULL)
  h == C_NULL && error("interpolate_traj_hip: run solve_gusto_hip! on this SCPSolution first")
  n, N = size(traj.X); m = size(traj.U, 1)
  X, U = Float64.(traj.X), Float64.(traj.U)
  nmax = Ref{Cint}(0)
  gusto_check(ccall((:gusto_interpolate, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GustoVerifyOpts}, Ref{Cint}),
                    h, X, U, GustoVerifyOpts(dt_min, 0, max(64, ceil(Int, traj.dt / dt_min)), 1), nmax), h, "interpolate")
  nfull, Xf, Uf = zeros(Cint, 1), zeros(n, nmax[]), zeros(m, nmax[] - 1)
  gusto_check(ccall((:gusto_get_dense, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}), h, nfull, Xf, Uf), h, "get_dense")
  Trajectory(Xf[:, 1:nfull[1]], Uf[:, 1:nfull[1]-1], traj.Tf)
end

# verify_collision_free(traj, SCPP) on the handle that solved SCPS: (free, k, dist) as the reference returns them
function verify_collision_free_hip(traj::Trajectory, SCPS::SCPSolution)
  h = get(GUSTO_HANDLES, SCPS, C_NULL)
  h == C_NULL && error("verify_collision_free_hip: run solve_gusto_hip! on this SCPSolution first")
  r = verify_batch!(h, 1, Float64.(traj.X), Float64.(traj.U); nstep=1, dense_collision=false)
  r.collision_free[1], r.first_knot[1], r.first_dist[1]
end

# ---- time-varying LQR tracking gains on the GPU (gusto_tvlqr, csrc/tvlqr.hip) ------------------------------------------------
# u = U[:,k] - K_k (x(t_k) - X[:,k]) around every trajectory of a handle, on the exact derivative of the zero-order-hold RK4
# roll-out gusto_interpolate performs (include/gusto_hip.h states the definitions; the reference has no counterpart).
# GuSTO handles only (TrajOpt handles answer GUSTO_ERR_ARG).
struct GustoTvlqrOpts      # gusto_tvlqr_opts
  Q::NTuple{13,Cdouble}; R::NTuple{6,Cdouble}; Qf::NTuple{13,Cdouble}
  dt_min::Cdouble; nstep::Cint; nstep_cap::Cint
  store_P::Cint
end
gusto_weights(w, dim, cap) = (v = w isa Number ? fill(Float64(w), dim) : Float64.(collect(w)); ntuple(i -> i <= dim ? v[i] : 0.0, cap))

# The gains of B problems of handle h (x_dim n, u_dim m, N knots); X [n,N,B], U [m,N,B] or nothing = the handle's own trajectories.
# Q, R, Qf: diagonal weights, numbers or vectors.  The C arrays are row-major, so the Julia arrays carry the transposes:
# K [n,m,N-1,B] with K[:,:,k,b]' = K_k, AB [n+m,n,N-1,B] with AB[:,:,k,b]' = [Ad_k Bd_k], P [n,n,B] of knot 1 or [n,n,N,B] with store_P.
function tvlqr_batch!(h::Ptr{Cvoid}, B::Integer, n::Integer, m::Integer, N::Integer, X=nothing, U=nothing; Q=1.0, R=1.0, Qf=1.0,
                      dt_min=0.1, nstep=0, nstep_cap=64, store_P=false)
  Xp = X === nothing ? Ptr{Cdouble}(C_NULL) : pointer(X); Up = U === nothing ? Ptr{Cdouble}(C_NULL) : pointer(U)
  o = GustoTvlqrOpts(gusto_weights(Q, n, 13), gusto_weights(R, m, 6), gusto_weights(Qf, n, 13), dt_min, nstep, nstep_cap, store_P ? 1 : 0)
  GC.@preserve X U gusto_check(ccall((:gusto_tvlqr, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GustoTvlqrOpts}),
                    h, Xp, Up, o), h, "tvlqr")
  status, fail_knot = zeros(Cint, B), zeros(Cint, B)
  K, AB = zeros(n, m, N - 1, B), zeros(n + m, n, N - 1, B)
  P = store_P ? zeros(n, n, N, B) : zeros(n, n, B)
  gusto_check(ccall((:gusto_get_tvlqr, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    h, status, fail_knot, K, P, AB), h, "get_tvlqr")
  ms = Ref{Cdouble}(0.0)
  gusto_check(ccall((:gusto_last_tvlqr_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, ms), h, "last_tvlqr_ms")
  (K = K, P = P, AB = AB, status = Int.(status), fail_knot = Int.(fail_knot), ms = ms[])
end

# ---- closed-loop Monte Carlo roll-outs of the tracking law on the GPU (gusto_simulate, csrc/simulate.hip) ---------------------
# Every trajectory of a handle flown n_samples times with its gains, from perturbed starts and with clipped controls
# (include/gusto_hip.h states the definitions; the reference has no counterpart).  GuSTO handles only.
struct GustoSimulateOpts      # gusto_simulate_opts
  n_samples::Cint
  seed::Culonglong; first_problem::Culonglong
  dx0::NTuple{13,Cdouble}; du0::NTuple{6,Cdouble}
  u_lo::NTuple{6,Cdouble}; u_hi::NTuple{6,Cdouble}
  dt_min::Cdouble; nstep::Cint; nstep_cap::Cint
  dense_collision::Cint
  store_knots::Cint
end
mutable struct GustoSimulateReport      # gusto_simulate_report
  n_free::Ptr{Cint}; n_finite::Ptr{Cint}; n_clipped::Ptr{Cint}; worst_sample::Ptr{Cint}; worst_dense_sample::Ptr{Cint}
  min_dist::Ptr{Cdouble}; max_dev::Ptr{Cdouble}; max_final_dev::Ptr{Cdouble}
  sample_min_dist::Ptr{Cdouble}
  sample_dense_index::Ptr{Cint}; sample_flags::Ptr{Cint}
  x_final::Ptr{Cdouble}
end
struct GustoDisturbOpts       # gusto_disturb_opts
  plant_rel::NTuple{6,Cdouble}; dw::NTuple{6,Cdouble}
end
gusto_bounds(w, dim, cap, off) = (v = w isa Number ? fill(Float64(w), dim) : Float64.(collect(w)); ntuple(i -> i <= dim ? v[i] : off, cap))

# The roll-outs of B problems of handle h (x_dim n, u_dim m, N knots).  X [n,N,B], U [m,N,B] or nothing = the handle's own
# trajectories; K [n,m,N-1,B] (K[:,:,k,b]' = K_k, as tvlqr_batch! returns it) or nothing = the gains of the last tvlqr_batch!;
# pert [n+m,S,B] or nothing = generated on the device.  The per-sample arrays come back as [S,B], x_final as [n,S,B], max_dev as
# [n,B]; with store_knots Xcl is [n,S,N,B].
# plant_rel (a number or the 6 half-widths of mass, Jdiag[1:3], dubins_v, dubins_k), dw (a number or m half-widths), plant [6,S,B]
# or white [m,S,N-1,B]: when any of them is given the roll-outs are those of gusto_simulate_disturbed -- the same law on a plant
# that differs per sample, with an actuator noise per hold interval -- and `plant` [6,S,B] comes back as well.
function simulate_batch!(h::Ptr{Cvoid}, B::Integer, n::Integer, m::Integer, N::Integer, X=nothing, U=nothing, K=nothing, pert=nothing;
                         n_samples=64, seed=0, first_problem=0, dx0=0.01, du0=0.0, u_lo=-Inf, u_hi=Inf, dt_min=0.1, nstep=0,
                         nstep_cap=64, dense_collision=true, store_knots=false, plant_rel=nothing, dw=nothing, plant=nothing,
                         white=nothing)
  ptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(a)
  S = Int(n_samples)
  o = GustoSimulateOpts(S, seed, first_problem, gusto_weights(dx0, n, 13), gusto_weights(du0, m, 6), gusto_bounds(u_lo, m, 6, -Inf),
                        gusto_bounds(u_hi, m, 6, Inf), dt_min, nstep, nstep_cap, dense_collision ? 1 : 0, store_knots ? 1 : 0)
  disturbed = !(plant_rel === nothing && dw === nothing && plant === nothing && white === nothing)
  if disturbed
    d = GustoDisturbOpts(gusto_weights(plant_rel === nothing ? 0.0 : plant_rel, 6, 6), gusto_weights(dw === nothing ? 0.0 : dw, m, 6))
    GC.@preserve X U K pert plant white gusto_check(ccall((:gusto_simulate_disturbed, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                       Ref{GustoSimulateOpts}, Ref{GustoDisturbOpts}),
                      h, ptr(X), ptr(U), ptr(K), ptr(pert), ptr(plant), ptr(white), o, d), h, "simulate_disturbed")
  else
    GC.@preserve X U K pert gusto_check(ccall((:gusto_simulate, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GustoSimulateOpts}),
                      h, ptr(X), ptr(U), ptr(K), ptr(pert), o), h, "simulate")
  end
  nfree, nfin, nclip, worst, wdense = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
  dmin, dev, fdev = zeros(B), zeros(n, B), zeros(n, B)
  sdist, sidx, sflags, xfin = zeros(S, B), zeros(Cint, S, B), zeros(Cint, S, B), zeros(n, S, B)
  GC.@preserve nfree nfin nclip worst wdense dmin dev fdev sdist sidx sflags xfin begin
    rep = GustoSimulateReport(pointer(nfree), pointer(nfin), pointer(nclip), pointer(worst), pointer(wdense), pointer(dmin),
                              pointer(dev), pointer(fdev), pointer(sdist), pointer(sidx), pointer(sflags), pointer(xfin))
    gusto_check(ccall((:gusto_get_simulate, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoSimulateReport}), h, rep), h, "get_simulate")
  end
  Xcl = store_knots ? zeros(n, S, N, B) : nothing
  store_knots && gusto_check(ccall((:gusto_get_simulate_knots, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, Xcl), h, "get_simulate_knots")
  used = disturbed ? zeros(6, S, B) : nothing
  disturbed && gusto_check(ccall((:gusto_get_simulate_plant, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, used), h, "get_simulate_plant")
  ms = Ref{Cdouble}(0.0)
  gusto_check(ccall((:gusto_last_simulate_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, ms), h, "last_simulate_ms")
  (n_free = Int.(nfree), n_finite = Int.(nfin), n_clipped = Int.(nclip), worst_sample = Int.(worst), worst_dense_sample = Int.(wdense),
   min_dist = dmin, max_dev = dev, max_final_dev = fdev, sample_min_dist = sdist, sample_dense_index = Int.(sidx),
   sample_flags = Int.(sflags), x_final = xfin, Xcl = Xcl, plant = used, ms = ms[])
end

# ---- linear covariance analysis with an uncertain plant (gusto_lincov_disturbed, csrc/lincov.hip) -------------------------------
# The covariance of z = [dx; b; theta - theta_nom] carried through the closed loop of every trajectory of a handle, to first order
# in the plant deviation (include/gusto_hip.h states the definitions; the reference has no counterpart).  After tvlqr_batch! on the
# same X, U.  GuSTO handles only.  These wrappers have not been run.
struct GustoLincovOpts      # gusto_lincov_opts
  dx0::NTuple{13,Cdouble}; du0::NTuple{6,Cdouble}; du_white::NTuple{6,Cdouble}
  u_lo::NTuple{6,Cdouble}; u_hi::NTuple{6,Cdouble}
  store_S::Cint
end
mutable struct GustoLincovReport      # gusto_lincov_report
  status::Ptr{Cint}; fail_knot::Ptr{Cint}; obs_knot::Ptr{Cint}; obs_pair::Ptr{Cint}; ctl_knot::Ptr{Cint}; ctl_entry::Ptr{Cint}
  min_z_obs::Ptr{Cdouble}; p_collision_bound::Ptr{Cdouble}; min_z_ctl::Ptr{Cdouble}
  sigma_x::Ptr{Cdouble}; sigma_u::Ptr{Cdouble}; z_obs::Ptr{Cdouble}; Sxx::Ptr{Cdouble}
end

# X [n,N,B], U [m,N,B] or nothing = the handle's own trajectories; K [n,m,N-1,B] or nothing = the gains of the last tvlqr_batch!;
# S0 [n+m,n+m,B] and Sth [6,6,B] (symmetric, so the transposes are themselves) or nothing = the default diagonals of dx0, du0 and
# plant_rel (a number or the 6 half-widths of mass, Jdiag[1:3], dubins_v, dubins_k); dw: a number or m half-widths of the noise per
# hold interval.  sigma_x comes back as [n,N,B], sigma_u as [m,N-1,B], z_obs as [N,B], Cd as [6,n,N-1,B] (Cd[:,:,k,b]' = Cd_k);
# with store_S Sxx [n,n,N,B] and Sxt [6,n,N,B].
function lincov_disturbed_batch!(h::Ptr{Cvoid}, B::Integer, n::Integer, m::Integer, N::Integer, X=nothing, U=nothing, K=nothing,
                                 S0=nothing, Sth=nothing; dx0=0.01, du0=0.0, du_white=0.0, u_lo=-Inf, u_hi=Inf, store_S=false,
                                 plant_rel=0.0, dw=0.0)
  ptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(a)
  o = GustoLincovOpts(gusto_weights(dx0, n, 13), gusto_weights(du0, m, 6), gusto_weights(du_white, m, 6), gusto_bounds(u_lo, m, 6, -Inf),
                      gusto_bounds(u_hi, m, 6, Inf), store_S ? 1 : 0)
  d = GustoDisturbOpts(gusto_weights(plant_rel, 6, 6), gusto_weights(dw, m, 6))
  GC.@preserve X U K S0 Sth gusto_check(ccall((:gusto_lincov_disturbed, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GustoLincovOpts}, Ref{GustoDisturbOpts}),
                    h, ptr(X), ptr(U), ptr(K), ptr(S0), ptr(Sth), o, d), h, "lincov_disturbed")
  status, fail_knot, obs_knot, obs_pair, ctl_knot, ctl_entry = (zeros(Cint, B) for _ in 1:6)
  zo, pb, zc = zeros(B), zeros(B), zeros(B)
  sx, su, z = zeros(n, N, B), zeros(m, N - 1, B), zeros(N, B)
  Sxx = store_S ? zeros(n, n, N, B) : nothing
  GC.@preserve status fail_knot obs_knot obs_pair ctl_knot ctl_entry zo pb zc sx su z Sxx begin
    rep = GustoLincovReport(pointer(status), pointer(fail_knot), pointer(obs_knot), pointer(obs_pair), pointer(ctl_knot), pointer(ctl_entry),
                            pointer(zo), pointer(pb), pointer(zc), pointer(sx), pointer(su), pointer(z), ptr(Sxx))
    gusto_check(ccall((:gusto_get_lincov, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoLincovReport}), h, rep), h, "get_lincov")
  end
  Cd = zeros(6, n, N - 1, B)
  Sxt = store_S ? zeros(6, n, N, B) : nothing
  GC.@preserve Cd Sxt gusto_check(ccall((:gusto_get_lincov_plant, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                    h, Cd, ptr(Sxt)), h, "get_lincov_plant")
  ms = Ref{Cdouble}(0.0)
  gusto_check(ccall((:gusto_last_lincov_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, ms), h, "last_lincov_ms")
  (status = Int.(status), fail_knot = Int.(fail_knot), obs_knot = Int.(obs_knot), obs_pair = Int.(obs_pair), ctl_knot = Int.(ctl_knot),
   ctl_entry = Int.(ctl_entry), min_z_obs = zo, p_collision_bound = pb, min_z_ctl = zc, sigma_x = sx, sigma_u = su, z_obs = z,
   Sxx = Sxx, Cd = Cd, Sxt = Sxt, ms = ms[])
end

# ---- obstacle margins at the dense samples between the knots (gusto_lincov_dense, csrc/lincov.hip) ------------------------------
# lincov_disturbed_batch!'s knot pass and, inside every hold interval, the position covariance at the samples of gusto_simulate /
# gusto_interpolate (the roll-out of the last tvlqr_batch!), turned into margins.  Same arguments; ws = 2 in the plane, 3 in space.
# Returns nfull, dense_sample (0-based, as the C ABI), dense_pair, min_z_dense [B] and, with store_dense, z_dense and pair_dense
# as [nfull_max,B] and Spos as [ws,ws,nfull_max,B]; gusto_get_lincov / gusto_get_lincov_plant then report the knot pass.  This
# wrapper has not been run.
mutable struct GustoLincovDenseReport      # gusto_lincov_dense_report
  nfull::Ptr{Cint}; dense_sample::Ptr{Cint}; dense_pair::Ptr{Cint}
  min_z_dense::Ptr{Cdouble}
  z_dense::Ptr{Cdouble}; pair_dense::Ptr{Cint}
  Spos::Ptr{Cdouble}
end
function lincov_dense_batch!(h::Ptr{Cvoid}, B::Integer, n::Integer, m::Integer, N::Integer, ws::Integer, X=nothing, U=nothing, K=nothing,
                             S0=nothing, Sth=nothing; dx0=0.01, du0=0.0, du_white=0.0, u_lo=-Inf, u_hi=Inf, store_S=false,
                             plant_rel=0.0, dw=0.0, store_dense=true)
  ptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(a)
  o = GustoLincovOpts(gusto_weights(dx0, n, 13), gusto_weights(du0, m, 6), gusto_weights(du_white, m, 6), gusto_bounds(u_lo, m, 6, -Inf),
                      gusto_bounds(u_hi, m, 6, Inf), store_S ? 1 : 0)
  d = GustoDisturbOpts(gusto_weights(plant_rel, 6, 6), gusto_weights(dw, m, 6))
  GC.@preserve X U K S0 Sth gusto_check(ccall((:gusto_lincov_dense, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GustoLincovOpts}, Ref{GustoDisturbOpts}, Cint),
                    h, ptr(X), ptr(U), ptr(K), ptr(S0), ptr(Sth), o, d, store_dense ? 1 : 0), h, "lincov_dense")
  rows = Ref{Cint}(0)
  gusto_check(ccall((:gusto_get_lincov_dense, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{GustoLincovDenseReport}, Ref{Cint}), h, C_NULL, rows),
              h, "get_lincov_dense")
  R = Int(rows[])
  nfull, js, jp = (zeros(Cint, B) for _ in 1:3)
  zmin = zeros(B)
  z = store_dense ? zeros(R, B) : nothing
  pr = store_dense ? zeros(Cint, R, B) : nothing
  Sp = store_dense ? zeros(ws, ws, R, B) : nothing
  GC.@preserve nfull js jp zmin z pr Sp begin
    rep = GustoLincovDenseReport(pointer(nfull), pointer(js), pointer(jp), pointer(zmin), ptr(z),
                                 pr === nothing ? Ptr{Cint}(C_NULL) : pointer(pr), ptr(Sp))
    gusto_check(ccall((:gusto_get_lincov_dense, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoLincovDenseReport}, Ptr{Cint}), h, rep, C_NULL),
                h, "get_lincov_dense")
  end
  ms = Ref{Cdouble}(0.0)
  gusto_check(ccall((:gusto_last_lincov_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, ms), h, "last_lincov_ms")
  (nfull = Int.(nfull), dense_sample = Int.(js), dense_pair = Int.(jp), min_z_dense = zmin, z_dense = z,
   pair_dense = pr === nothing ? nothing : Int.(pr), Spos = Sp, nfull_max = R, ms = ms[])
end

# ---- multi-start solves: a fan of detour starts per query, best-of-K select (csrc/multistart.hip) ------------------------------
# GuSTO is a local method: every TOP is one planning QUERY, started from K initial trajectories in the same launch -- the straight
# line bent sideways by fan[:, j] = (a2, a3) metres (gusto_set_problems_multistart; include/gusto_hip.h states the definitions, the
# reference has no counterpart) -- and answered with the best start that is converged and successful (gusto_select_best on the last
# true cost).  policy = :all: one launch of B K problems; :retry: a plain straight-line solve first, then the fan for the queries
# that are not successful only, on the same handle; a query solved in the first pass keeps that result.  Returns per query
# (winner, cost): the winning start (1-based; 0 = none qualified) and its cost (Inf likewise); TOSs[q] receives the winner's
# solution, without one the straight line's.  All TOPs share model, N and the environment.  Mirrors gusto.jl_amd/host.py:
# solve_SCP_multistart_batch.  This wrapper has not been run.
const GUSTO_MAX_STARTS = 64
mutable struct GustoBestReport      # gusto_best_report
  winner::Ptr{Cint}; winner_problem::Ptr{Cint}; n_eligible::Ptr{Cint}
  best_score::Ptr{Cdouble}
  X::Ptr{Cdouble}; U::Ptr{Cdouble}
end
gusto_default_fan(model) = gusto_model_id(model) in (0, 1) ? [0. .5 -.5 1. -1.; 0. 0. 0. 0. 0.] : [0. .5 -.5 0. 0.; 0. 0. 0. .5 -.5]

function solve_SCP_multistart_batch!(TOSs::Vector, TOPs::Vector; fan=nothing, policy=:all, max_iter=30, force=false, device=0)
  policy in (:all, :retry) || error("solve_SCP_multistart_batch!: policy is :all or :retry")
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, Q = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N && T.PD.env === TOP0.PD.env, TOPs) ||
    error("solve_SCP_multistart_batch!: all problems must share the model type, N and the environment")
  F = fan === nothing ? gusto_default_fan(model) : Matrix{Float64}(fan)      # [2, K]: column j = (a2, a3) of start j
  K = size(F, 2)
  cap = policy == :all ? Q * K : max(Q, K)
  alg0 = SCPParam_GuSTO(model)
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail,
                      SCPParam(model, TOP0.fixed_final_time).convergence_threshold)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, cap, gusto_hist_cap(max_iter), device), href[], "create")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                    h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
  boxes, spheres = gusto_env_tables(TOP0.PD.env)
  gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                    h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat(first.(bounds)...), hcat(last.(bounds)...)
  tf = Float64[T.tf_guess for T in TOPs]
  result = [(0, Inf) for _ in 1:Q]

  # everything a solution needs from the B problems the handle holds now, after gusto_solve(max_iter)
  function solve_and_fetch(B)
    gusto_check(ccall((:gusto_solve, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, max_iter, force), h, "solve")
    X, U = zeros(n, N, B), zeros(m, N, B)
    gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
    its, conv, succ, stop = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
    gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}),
                      h, its, conv, succ, stop, C_NULL), h, "get_status")
    duals = zeros(n, B)
    gusto_check(ccall((:gusto_get_dual, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, duals), h, "get_dual")
    msec = Ref{Cdouble}(0.)
    ccall((:gusto_last_solve_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, msec)
    (X = X, U = U, its = its, conv = conv, succ = succ, stop = stop, duals = duals, Hs = gusto_histories(h, B), per = msec[] / 1e3 / B)
  end
  function take!(q, S, j, winner, cost)       # problem j of the snapshot S answers query q
    SCPP = SCPProblem(TOPs[q])
    SCPP.param.alg = SCPParam_GuSTO(model)
    SCPS = SCPSolution(SCPP, Trajectory(S.X[:, :, j], S.U[:, :, j], TOPs[q].tf_guess))
    gusto_fill_solution!(SCPS, SCPP.param.alg, S.Hs, j, S.its[j], S.conv[j], S.succ[j], S.stop[j], S.duals[:, j])
    SCPS.total_time = S.per
    SCPS.iter_elapsed_times = vcat(0., fill(SCPS.total_time / max(1, S.its[j]), S.its[j]))
    SCPP.param.obstacle_toggle_distance = SCPP.param.alg.Δ_vec[end] / 8 + model.clearance
    TOSs[q].traj, TOSs[q].SCPS = SCPS.traj, SCPS
    result[q] = (winner, cost)
  end
  function fanned!(qs, keep_loser)             # the queries qs through one fanned launch
    Bq = length(qs)
    gusto_check(ccall((:gusto_set_problems_multistart, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                      h, Bq, K, x0[:, qs], lo[:, qs], hi[:, qs], tf[qs], F), h, "set_problems_multistart")
    S = solve_and_fetch(Bq * K)
    gusto_check(ccall((:gusto_select_best, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cint}), h, K, C_NULL, C_NULL), h, "select_best")
    win, wp, best = zeros(Cint, Bq), zeros(Cint, Bq), zeros(Bq)
    GC.@preserve win wp best begin
      rep = GustoBestReport(pointer(win), pointer(wp), C_NULL, pointer(best), C_NULL, C_NULL)
      gusto_check(ccall((:gusto_get_best, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoBestReport}), h, rep), h, "get_best")
    end
    for (i, q) in enumerate(qs)
      if win[i] >= 0
        take!(q, S, wp[i] + 1, win[i] + 1, best[i])
      elseif keep_loser
        take!(q, S, (i - 1) * K + 1, 0, Inf)
      end
    end
  end

  if policy == :all
    fanned!(collect(1:Q), true)
  else
    gusto_check(ccall((:gusto_set_problems, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                      h, Q, x0, lo, hi, tf, C_NULL, C_NULL), h, "set_problems")      # X0 = NULL: init_traj_straightline on the device
    S = solve_and_fetch(Q)
    ok = [S.conv[q] != 0 && S.succ[q] != 0 for q in 1:Q]
    for q in 1:Q
      take!(q, S, q, ok[q] ? 1 : 0, ok[q] ? TOSs[q].SCPS.J_true[end] : Inf)
    end
    again = findall(.!ok)
    per = cap ÷ K
    for c in 1:per:length(again)
      fanned!(again[c:min(c + per - 1, length(again))], false)
    end
  end
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  result
end

# ---- trajectory library: every query seeded from its nearest solved neighbours (csrc/trajlib.hip) ------------------------------
# GuSTO is warm-started at its previous iterate: a query that starts from the solved trajectory of a similar query needs fewer
# trips than one that starts from the straight line.  A gusto_trajlib keeps solved trajectories on the device;
# gusto_set_problems_trajlib finds the K nearest entries of every query and retargets them to its end points (include/gusto_hip.h
# states the definitions, the reference has no counterpart).  TrajLib owns one library; trajlib_add! appends the converged and
# successful (or the masked) problems of a handle device to device, trajlib_get / trajlib_add_host! move a library through host
# arrays ([x_dim, L], [x_dim, N, L], [u_dim, N, L]: the column-major images of the C rows).  solve_SCP_trajlib_batch! seeds,
# solves and selects; with fallback_fan the queries without a winner go through solve_SCP_multistart_batch!'s fan afterwards;
# with learn the winners join the library.  Returns per query (winner, cost, entry): the winning start (1-based; 0 = none
# qualified), its cost (Inf likewise) and the library entry it was seeded from (1-based; 0 = a straight line or a fan start).
# Mirrors gusto.jl_amd/host.py: TrajLib, solve_SCP_trajlib_batch.  This wrapper has not been run.
const GUSTO_TRAJLIB_MAX_K = 8
struct GustoTrajlibOpts      # gusto_trajlib_opts
  w_init::NTuple{13,Cdouble}; w_goal::NTuple{13,Cdouble}
  w_tf::Cdouble
  lds_tile::Cint
end
mutable struct TrajLib
  h::Ptr{Cvoid}; model_id::Int; n::Int; m::Int; N::Int; cap::Int; device::Int
end
trajlib_check(rc, lib, what) = rc == 0 || error("gusto_trajlib_$what -> $rc: " *
  unsafe_string(ccall((:gusto_trajlib_last_error, libgusto_hip), Cstring, (Ptr{Cvoid},), lib)))

function TrajLib(model, N::Integer, cap::Integer; device=0, w_init=nothing, w_goal=nothing, w_tf=nothing)
  id, n, m = gusto_model_id(model), model.x_dim, model.u_dim
  o = Ref(GustoTrajlibOpts(ntuple(_ -> 0., 13), ntuple(_ -> 0., 13), 0., 1))
  ccall((:gusto_default_trajlib_opts, libgusto_hip), Cint, (Cint, Ref{GustoTrajlibOpts}), id, o) == 0 || error("gusto_default_trajlib_opts")
  pad(w, d) = w === nothing ? d : ntuple(i -> i <= n ? Float64(w isa Number ? w : w[i]) : 0., 13)
  o[] = GustoTrajlibOpts(pad(w_init, o[].w_init), pad(w_goal, o[].w_goal), w_tf === nothing ? o[].w_tf : Float64(w_tf), o[].lds_tile)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  trajlib_check(ccall((:gusto_trajlib_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Ref{GustoTrajlibOpts}),
                      href, id, N, cap, device, o), C_NULL, "create")
  TrajLib(href[], id, n, m, N, cap, device)
end
trajlib_destroy!(lib::TrajLib) = (ccall((:gusto_trajlib_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), lib.h); lib.h = C_NULL; nothing)
trajlib_clear!(lib::TrajLib) = trajlib_check(ccall((:gusto_trajlib_clear, libgusto_hip), Cint, (Ptr{Cvoid},), lib.h), lib.h, "clear")
function Base.length(lib::TrajLib)
  c = Ref{Cint}(0)
  trajlib_check(ccall((:gusto_trajlib_size, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Cint}), lib.h, c, C_NULL), lib.h, "size")
  Int(c[])
end
# the problems of handle h (B of them) whose mask is nonzero (nothing: converged and successful); returns the number appended
function trajlib_add!(lib::TrajLib, h::Ptr{Cvoid}, B::Integer; mask=nothing, tag=nothing)
  mk = mask === nothing ? C_NULL : Cint.(mask .!= 0)
  tg = tag === nothing ? C_NULL : (tag isa Number ? fill(Cint(tag), B) : Cint.(tag))
  added = Ref{Cint}(0)
  trajlib_check(ccall((:gusto_trajlib_add, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ref{Cint}),
                      lib.h, h, mk, tg, added), lib.h, "add")
  Int(added[])
end
function trajlib_add_host!(lib::TrajLib, x_init, goal_lo, goal_hi, tf, X, U; tag=nothing)
  L = length(tf)
  tg = tag === nothing ? C_NULL : Cint.(tag)
  trajlib_check(ccall((:gusto_trajlib_add_host, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}),
                      lib.h, L, Matrix{Float64}(x_init), Matrix{Float64}(goal_lo), Matrix{Float64}(goal_hi), Vector{Float64}(tf), tg,
                      Array{Float64}(X), Array{Float64}(U)), lib.h, "add_host")
end
function trajlib_get(lib::TrajLib)
  L = length(lib)
  x_init, goal_c, tf, tag = zeros(lib.n, L), zeros(lib.n, L), zeros(L), zeros(Cint, L)
  X, U = zeros(lib.n, lib.N, L), zeros(lib.m, lib.N, L)
  trajlib_check(ccall((:gusto_trajlib_get, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}),
                      lib.h, x_init, goal_c, tf, tag, X, U), lib.h, "get")
  (x_init = x_init, goal_c = goal_c, tf = tf, tag = Int.(tag), X = X, U = U)
end

function solve_SCP_trajlib_batch!(TOSs::Vector, TOPs::Vector, lib::TrajLib; K=1, fallback_fan=nothing, learn=false, max_iter=30,
                                  force=false)
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, Q = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N && T.PD.env === TOP0.PD.env, TOPs) ||
    error("solve_SCP_trajlib_batch!: all problems must share the model type, N and the environment")
  (gusto_model_id(model) == lib.model_id && N == lib.N) || error("solve_SCP_trajlib_batch!: the library belongs to another model or N")
  1 <= K <= GUSTO_TRAJLIB_MAX_K || error("solve_SCP_trajlib_batch!: K outside 1 .. GUSTO_TRAJLIB_MAX_K")
  alg0 = SCPParam_GuSTO(model)
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail,
                      SCPParam(model, TOP0.fixed_final_time).convergence_threshold)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, Q * K, gusto_hist_cap(max_iter), lib.device), href[], "create")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                    h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
  boxes, spheres = gusto_env_tables(TOP0.PD.env)
  gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                    h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat(first.(bounds)...), hcat(last.(bounds)...)
  tf = Float64[T.tf_guess for T in TOPs]
  B = Q * K
  gusto_check(ccall((:gusto_set_problems_trajlib, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                    h, lib.h, Q, K, x0, lo, hi, tf, C_NULL), h, "set_problems_trajlib")
  entry, nfound = zeros(Cint, K, Q), zeros(Cint, Q)
  gusto_check(ccall((:gusto_get_trajlib_seeds, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}),
                    h, entry, C_NULL, nfound), h, "get_trajlib_seeds")
  gusto_check(ccall((:gusto_solve, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, max_iter, force), h, "solve")
  X, U = zeros(n, N, B), zeros(m, N, B)
  gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
  its, conv, succ, stop = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
  gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}),
                    h, its, conv, succ, stop, C_NULL), h, "get_status")
  duals = zeros(n, B)
  gusto_check(ccall((:gusto_get_dual, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, duals), h, "get_dual")
  msec = Ref{Cdouble}(0.)
  ccall((:gusto_last_solve_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, msec)
  Hs = gusto_histories(h, B)
  gusto_check(ccall((:gusto_select_best, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cint}), h, K, C_NULL, C_NULL), h, "select_best")
  win, wp, best = zeros(Cint, Q), zeros(Cint, Q), zeros(Q)
  GC.@preserve win wp best begin
    rep = GustoBestReport(pointer(win), pointer(wp), C_NULL, pointer(best), C_NULL, C_NULL)
    gusto_check(ccall((:gusto_get_best, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoBestReport}), h, rep), h, "get_best")
  end
  result = Vector{Any}(undef, Q)
  for q in 1:Q
    j = win[q] >= 0 ? wp[q] + 1 : (q - 1) * K + 1      # without a winner: start 1 of the query
    SCPP = SCPProblem(TOPs[q])
    SCPP.param.alg = SCPParam_GuSTO(model)
    SCPS = SCPSolution(SCPP, Trajectory(X[:, :, j], U[:, :, j], TOPs[q].tf_guess))
    gusto_fill_solution!(SCPS, SCPP.param.alg, Hs, j, its[j], conv[j], succ[j], stop[j], duals[:, j])
    SCPS.total_time = msec[] / 1e3 / B
    SCPS.iter_elapsed_times = vcat(0., fill(SCPS.total_time / max(1, its[j]), its[j]))
    SCPP.param.obstacle_toggle_distance = SCPP.param.alg.Δ_vec[end] / 8 + model.clearance
    TOSs[q].traj, TOSs[q].SCPS = SCPS.traj, SCPS
    result[q] = win[q] >= 0 ? (win[q] + 1, best[q], entry[win[q] + 1, q] + 1) : (0, Inf, 0)
  end
  if learn && any(win .>= 0)
    mask = zeros(Cint, B)
    mask[wp[win .>= 0] .+ 1] .= 1
    trajlib_add!(lib, h, B; mask=mask)
  end
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  lost = findall(win .< 0)
  if fallback_fan !== nothing && !isempty(lost)      # the multi-start path for the queries the library could not answer
    fan = fallback_fan === true ? nothing : fallback_fan
    again = solve_SCP_multistart_batch!(TOSs[lost], TOPs[lost]; fan=fan, policy=:all, max_iter=max_iter, force=force, device=lib.device)
    for (i, q) in enumerate(lost)
      again[i][1] > 0 && (result[q] = (again[i][1], again[i][2], 0))
    end
  end
  result
end

# ---- receding-horizon replanning: a batch restarted from where each plan is (csrc/replan.hip) -----------------------------------
# After a few knots of flight the robot is not on its plan: gusto_set_problems_replan makes, of every problem of a handle, a new one
# from the measured state to the same goals in the time that is left, tf' = (1 - tau) tf, started from the solved plan shifted in
# time and bent to the new start (include/gusto_hip.h states the definitions, the reference has no counterpart).
# Mirrors gusto.jl_amd/host.py: replan_batch, solve_SCP_receding_batch.  This wrapper has not been run.
const GUSTO_REPLAN_TRAJ, GUSTO_REPLAN_BEST = 0, 1

# B problems of handle h (x_dim n) replanned from the states x_now [n,B] after the fractions tau [B] of their time.  src: the handle
# that holds the plans (C_NULL: h itself; its N may differ); source :traj = problem b of src, :best = query b of its last
# gusto_select_best.  tf_s [B] or nothing: the tf of the source problems, for the reference's only row on the final time,
# Tf >= 0.1, checked on tf'.  goal_lo / goal_hi [n,B] or nothing = the source's goals; mask [B] or nothing = the converged and
# successful plans (the queries with a winner) are seeded, the others start from the straight line.
# Returns (seeded [B], tau [B], x_now [n,B], ms).
function replan_batch!(h::Ptr{Cvoid}, B::Integer, n::Integer, tau, x_now; src::Ptr{Cvoid}=Ptr{Cvoid}(C_NULL), source=:traj, tf_s=nothing,
                       goal_lo=nothing, goal_hi=nothing, mask=nothing)
  source in (:traj, :best) || error("replan_batch!: source is :traj or :best")
  (goal_lo === nothing) == (goal_hi === nothing) || error("replan_batch!: goal_lo and goal_hi are given together or not at all")
  t = tau isa Number ? fill(Float64(tau), B) : Float64.(collect(tau))
  tf_s === nothing || all((1 .- t) .* tf_s .>= 0.1) ||
    error("replan_batch!: tf' = (1 - tau) tf violates the only row on Tf, Tf >= 0.1 (scp_gusto.jl:248-250)")
  x = Matrix{Float64}(x_now)
  lo = goal_lo === nothing ? nothing : Matrix{Float64}(goal_lo); hi = goal_hi === nothing ? nothing : Matrix{Float64}(goal_hi)
  mk = mask === nothing ? nothing : Cint.(mask .!= 0)
  ptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(a)
  GC.@preserve t x lo hi mk gusto_check(ccall((:gusto_set_problems_replan, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                    h, src, source == :best ? GUSTO_REPLAN_BEST : GUSTO_REPLAN_TRAJ, B, t, x, ptr(lo), ptr(hi),
                    mk === nothing ? Ptr{Cint}(C_NULL) : pointer(mk)), h, "set_problems_replan")
  gusto_replan_info(h, B, n)
end

function gusto_replan_info(h::Ptr{Cvoid}, B::Integer, n::Integer)
  seeded, t, x = zeros(Cint, B), zeros(B), zeros(n, B)
  gusto_check(ccall((:gusto_get_replan, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}), h, seeded, t, x), h, "get_replan")
  ms = Ref{Cdouble}(0.0)
  gusto_check(ccall((:gusto_last_replan_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, ms), h, "last_replan_ms")
  (seeded = seeded .!= 0, tau = t, x_now = x, ms = ms[])
end

# A receding-horizon loop on one handle.  Per step: gusto_solve, the gains (tvlqr_batch!), the flight (simulate_batch! as
# gusto_simulate_disturbed with two samples and store_knots: sample 1 of the C ABI is the first perturbed one), then
# gusto_set_problems_replan_knots with knot = knots_per_step and sample = 1: the next step plans from where the roll-out is, to the
# same goals, in the time that is left.  All TOPs share model, N and the environment.  Returns one named tuple per step:
# iterations, converged, successful [B], solve_ms of the step's solve; x_now [n,B], tau [B], seeded [B], replan_ms of the replan
# that ends it.  TOSs take the last plan.
function solve_SCP_receding_batch!(TOSs::Vector, TOPs::Vector, steps::Integer, knots_per_step::Integer; plant_rel=0.0, dw=0.0, dx0=0.01,
                                   Q=1.0, R=1.0, Qf=1.0, max_iter=30, force=false, device=0)
  length(TOSs) == length(TOPs) && !isempty(TOPs) || error("solve_SCP_receding_batch!: need as many solutions as problems, at least one")
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, B = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N && T.PD.env === TOP0.PD.env, TOPs) ||
    error("solve_SCP_receding_batch!: all problems must share the model type, N and the environment")
  (steps >= 1 && 0 <= knots_per_step <= N - 2) || error("solve_SCP_receding_batch!: need steps >= 1 and 0 <= knots_per_step <= N - 2")
  alg0 = SCPParam_GuSTO(model)
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail,
                      SCPParam(model, TOP0.fixed_final_time).convergence_threshold)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, B, gusto_hist_cap(max_iter), device), href[], "create")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                    h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
  boxes, spheres = gusto_env_tables(TOP0.PD.env)
  gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                    h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat(first.(bounds)...), hcat(last.(bounds)...)
  tf = Float64[T.tf_guess for T in TOPs]
  gusto_check(ccall((:gusto_set_problems, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    h, B, x0, lo, hi, tf, C_NULL, C_NULL), h, "set_problems")
  tau = knots_per_step / (N - 1)
  knot = fill(Cint(knots_per_step), B)
  out = Vector{Any}(undef, steps)
  X, U = zeros(n, N, B), zeros(m, N, B)
  its, conv, succ, stop = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
  duals = zeros(n, B)
  msec = Ref{Cdouble}(0.)
  Hs = nothing
  tf_plan = copy(tf)
  for s in 1:steps
    tf_plan = copy(tf)
    gusto_check(ccall((:gusto_solve, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, max_iter, force), h, "solve")
    gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
    gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}),
                      h, its, conv, succ, stop, C_NULL), h, "get_status")
    gusto_check(ccall((:gusto_get_dual, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, duals), h, "get_dual")
    ccall((:gusto_last_solve_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, msec)
    Hs = gusto_histories(h, B)
    tvlqr_batch!(h, B, n, m, N; Q=Q, R=R, Qf=Qf)
    simulate_batch!(h, B, n, m, N; n_samples=2, dx0=dx0, store_knots=true, plant_rel=plant_rel, dw=dw)
    tf = (1 - tau) .* tf
    all(tf .>= 0.1) || error("solve_SCP_receding_batch!: tf' = (1 - tau) tf violates the only row on Tf, Tf >= 0.1 (scp_gusto.jl:248-250)")
    gusto_check(ccall((:gusto_set_problems_replan_knots, libgusto_hip), Cint,
                      (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cint}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                      h, C_NULL, B, knot, 1, C_NULL, C_NULL, C_NULL), h, "set_problems_replan_knots")
    info = gusto_replan_info(h, B, n)
    out[s] = (iterations = Int.(its), converged = conv .!= 0, successful = succ .!= 0, solve_ms = msec[], x_now = info.x_now,
              tau = info.tau, seeded = info.seeded, replan_ms = info.ms)
  end
  for q in 1:B
    SCPP = SCPProblem(TOPs[q])
    SCPP.param.alg = SCPParam_GuSTO(model)
    SCPS = SCPSolution(SCPP, Trajectory(X[:, :, q], U[:, :, q], tf_plan[q]))
    gusto_fill_solution!(SCPS, SCPP.param.alg, Hs, q, its[q], conv[q], succ[q], stop[q], duals[:, q])
    SCPS.total_time = msec[] / 1e3 / B
    SCPS.iter_elapsed_times = vcat(0., fill(SCPS.total_time / max(1, its[q]), its[q]))
    SCPP.param.obstacle_toggle_distance = SCPP.param.alg.Δ_vec[end] / 8 + model.clearance
    TOSs[q].traj, TOSs[q].SCPS = SCPS.traj, SCPS
  end
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  out
end

# ---- risk-tightened keep-out sets: plan to a margin in standard deviations (csrc/tighten.hip) ------------------------------------
# gusto_lincov reports how many standard deviations of closed-loop dispersion lie between a plan and the nearest keep-out
# component; gusto_tighten_env feeds that back: from the BASE tables and the covariances of the last gusto_lincov (store_S = 1) it
# writes per-problem tables -- every component extended over the robot's component offsets, then grown by kappa sigma_d -- where
# gusto_set_env_batch puts its own (include/gusto_hip.h states the definitions, the reference has no counterpart).
# Mirrors gusto.jl_amd/host.py: BatchSolver.tighten_env, solve_SCP_chance_batch.  This wrapper has not been run.
struct GustoTightenOpts      # gusto_tighten_opts
  kappa::Cdouble; slack::Cdouble; margin_cap::Cdouble; reach::Cdouble; cover_components::Cint; monotone::Cint
end
mutable struct GustoTightenReport      # gusto_tighten_report
  status::Ptr{Cint}; knot::Ptr{Cint}; pair::Ptr{Cint}; n_grown::Ptr{Cint}; blocked::Ptr{Cint}
  min_z_base::Ptr{Cdouble}; max_margin::Ptr{Cdouble}; margin::Ptr{Cdouble}
end

# boxes / spheres: vectors of [6,n_box] / [4,n_sph] tables, of length 1 (one base set for the batch) or B.
# Returns (status, knot, pair, n_grown, blocked, min_z_base, max_margin [B], margin [n_obs_max,B], ms).
function tighten_env!(h::Ptr{Cvoid}, B::Integer, boxes::Vector, spheres::Vector; kappa=3.0, slack=0.0, margin_cap=Inf, reach=Inf,
                      cover_components=true, monotone=true)
  length(boxes) == length(spheres) && length(boxes) in (1, B) || error("tighten_env!: one base set, or one per problem")
  nb, ns = Cint[length(b) ÷ 6 for b in boxes], Cint[length(s) ÷ 4 for s in spheres]
  box = Float64.(vcat((vec(b) for b in boxes)..., Float64[])); sph = Float64.(vcat((vec(s) for s in spheres)..., Float64[]))
  o = GustoTightenOpts(kappa, slack, margin_cap, reach, cover_components ? 1 : 0, monotone ? 1 : 0)
  gusto_check(ccall((:gusto_tighten_env, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ref{GustoTightenOpts}),
                    h, length(boxes), nb, box, ns, sph, o), h, "tighten_env")
  w = Ref{Cint}(0)
  gusto_check(ccall((:gusto_get_tighten, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cint}), h, C_NULL, w), h, "get_tighten")
  st, kn, pr, ng, bl = (zeros(Cint, B) for _ in 1:5)
  mz, mm, mg = zeros(B), zeros(B), zeros(Int(w[]), B)
  GC.@preserve st kn pr ng bl mz mm mg begin
    rep = GustoTightenReport(pointer(st), pointer(kn), pointer(pr), pointer(ng), pointer(bl), pointer(mz), pointer(mm), pointer(mg))
    gusto_check(ccall((:gusto_get_tighten, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoTightenReport}, Ptr{Cint}), h, rep, C_NULL), h, "get_tighten")
  end
  ms = Ref{Cdouble}(0.0)
  gusto_check(ccall((:gusto_last_tighten_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, ms), h, "last_tighten_ms")
  (status = st, knot = kn, pair = pr, n_grown = ng, blocked = bl .!= 0, min_z_base = mz, max_margin = mm, margin = mg, ms = ms[])
end

# The handle's current keep-out tables: (n_box [n_env], boxes [6, sum n_box], n_sph [n_env], spheres [4, sum n_sph])
function gusto_env(h::Ptr{Cvoid})
  ne = Ref{Cint}(0)
  gusto_check(ccall((:gusto_get_env, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}),
                    h, ne, C_NULL, C_NULL, C_NULL, C_NULL), h, "get_env")
  nb, ns = zeros(Cint, ne[]), zeros(Cint, ne[])
  gusto_check(ccall((:gusto_get_env, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}),
                    h, C_NULL, nb, C_NULL, ns, C_NULL), h, "get_env")
  box, sph = zeros(6, sum(nb)), zeros(4, sum(ns))
  gusto_check(ccall((:gusto_get_env, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}),
                    h, C_NULL, C_NULL, box, C_NULL, sph), h, "get_env")
  (n_box = nb, boxes = box, n_sph = ns, spheres = sph)
end

# Plans that keep kappa standard deviations from every keep-out component, on one handle: solve; per round the gains
# (tvlqr_batch!), the covariances (lincov_disturbed_batch! with store_S), tighten_env! from the base set for the answered
# problems below kappa (gusto_set_active), a re-solve of those from their own plan (replan_batch! with tau = 0, x_now = x_init)
# and once more from the straight line for the ones that pass loses; at the end the base set again and the analysis on it.  All
# TOPs share model, N and the environment.  A problem that loses both passes keeps its last answered plan.  Returns
# (answered, met [B], min_z_obs [B], rounds = one named tuple per round).  TOSs take the final trajectories.
function solve_SCP_chance_batch!(TOSs::Vector, TOPs::Vector; kappa=3.0, rounds=3, dx0=0.01, du_white=0.0, plant_rel=0.0, dw=0.0,
                                 Q=1.0, R=1.0, Qf=1.0, max_iter=30, force=false, device=0)
  length(TOSs) == length(TOPs) && !isempty(TOPs) || error("solve_SCP_chance_batch!: need as many solutions as problems, at least one")
  any(!iszero, du_white) || any(!iszero, plant_rel) || any(!iszero, dw) ||
    error("solve_SCP_chance_batch!: du_white is all zero and no plant dispersion is given: the covariance decays to rounding noise")
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, B = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N && T.PD.env === TOP0.PD.env, TOPs) ||
    error("solve_SCP_chance_batch!: all problems must share the model type, N and the environment")
  alg0 = SCPParam_GuSTO(model)
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail,
                      SCPParam(model, TOP0.fixed_final_time).convergence_threshold)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, B, gusto_hist_cap(max_iter), device), href[], "create")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                    h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
  boxes, spheres = gusto_env_tables(TOP0.PD.env)
  set_base() = gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                                 h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
  set_base()
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat(first.(bounds)...), hcat(last.(bounds)...)
  tf = Float64[T.tf_guess for T in TOPs]
  gusto_check(ccall((:gusto_set_problems, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    h, B, x0, lo, hi, tf, C_NULL, C_NULL), h, "set_problems")
  X, U = zeros(n, N, B), zeros(m, N, B)
  its, conv, succ, stop = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
  function solve_active!(active)
    mask = active === nothing ? nothing : Cint.(active)
    gusto_check(ccall((:gusto_set_active, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}), h, mask === nothing ? C_NULL : mask), h, "set_active")
    gusto_check(ccall((:gusto_solve, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, max_iter, force), h, "solve")
    gusto_check(ccall((:gusto_set_active, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}), h, C_NULL), h, "set_active")
    gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
    gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}),
                      h, its, conv, succ, stop, C_NULL), h, "get_status")
    (conv .!= 0) .& (succ .!= 0)
  end
  analyse!() = (tvlqr_batch!(h, B, n, m, N, keepX, keepU; Q=Q, R=R, Qf=Qf);
                lincov_disturbed_batch!(h, B, n, m, N, keepX, keepU; dx0=dx0, du_white=du_white, plant_rel=plant_rel, dw=dw, store_S=true))
  answered = solve_active!(nothing)
  keepX, keepU = copy(X), copy(U)
  onh, done, stuck = trues(B), falses(B), falses(B)
  out = Any[]
  for r in 1:rounds
    open = answered .& .!done .& .!stuck
    any(open) || break
    analyse!()
    gusto_check(ccall((:gusto_set_active, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}), h, Cint.(open)), h, "set_active")
    rep = tighten_env!(h, B, [boxes], [spheres]; kappa=kappa)
    gusto_check(ccall((:gusto_set_active, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}), h, C_NULL), h, "set_active")
    done .|= open .& (rep.min_z_base .>= kappa)
    todo = open .& .!done .& .!rep.blocked
    stuck .|= open .& .!done .& rep.blocked
    lost = falses(B)
    if any(todo)
      replan_batch!(h, B, n, 0.0, x0; mask=onh)
      win = todo .& solve_active!(todo)
      keepX[:, :, win], keepU[:, :, win] = X[:, :, win], U[:, :, win]
      again = todo .& .!win
      onh[again] .= false
      if any(again)
        replan_batch!(h, B, n, 0.0, x0; mask=onh)
        win2 = again .& solve_active!(again)
        keepX[:, :, win2], keepU[:, :, win2] = X[:, :, win2], U[:, :, win2]
        onh[win2] .= true
        lost = again .& .!win2
        stuck .|= lost
      end
    end
    push!(out, (tried = todo, min_z_base = rep.min_z_base, max_margin = rep.max_margin, blocked = rep.blocked, lost = lost, tighten_ms = rep.ms))
  end
  set_base()
  lc = analyse!()
  for q in 1:B
    TOSs[q].traj = Trajectory(keepX[:, :, q], keepU[:, :, q], tf[q])
  end
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  (answered = answered, met = answered .& (lc.min_z_obs .>= kappa), min_z_obs = lc.min_z_obs, rounds = out)
end

# ---- roadmap seeds: every query starts from a shortest collision-free polyline (csrc/roadmap.hip) -------------------------------
# None of the fan, the library and replanning looks at the keep-out set before the first solve; gusto_set_problems_roadmap does:
# a visibility graph over the corners of the inflated keep-out components, per query the shortest path and, as alternates, the
# shortest paths that avoid the corners of one more component each; the polyline resampled by arc length is the initial
# trajectory (a query with an unblocked line, or without a path, is the straight line).  include/gusto_hip.h states the
# definitions; the reference has no counterpart.  Mirrors gusto.jl_amd/host.py: BatchSolver.set_problems_roadmap,
# solve_SCP_roadmap_batch.  This wrapper has not been run.
const GUSTO_ROADMAP_MAX_K = 8
const GUSTO_ROADMAP_MAX_VIA = 16
struct GustoRoadmapOpts      # gusto_roadmap_opts
  inflate::Cdouble; pad::Cdouble
  straight_first::Cint
end
mutable struct GustoRoadmapReport      # gusto_roadmap_report
  status::Ptr{Cint}; n_via::Ptr{Cint}
  via::Ptr{Cint}
  length::Ptr{Cdouble}
  banned::Ptr{Cint}
  stage_ms::Ptr{Cdouble}
end

# Bq queries (columns of x0, lo, hi; tf [Bq]) x K alternates become the B = Bq K problems of the handle h, problem (q - 1) K + j
# = alternate j of query q, from the handle's current keep-out tables.  inflate / pad = nothing: the model's defaults.  Returns
# (status, n_via, via [16, B], length, banned [8, B], stage_ms = (graph, search, seed), ms)
function set_problems_roadmap!(h::Ptr{Cvoid}, model_id::Integer, x0::Matrix{Float64}, lo::Matrix{Float64}, hi::Matrix{Float64}, tf::Vector{Float64};
                               K=1, inflate=nothing, pad=nothing, straight_first=false)
  Bq = size(x0, 2); B = Bq * K
  d = Ref(GustoRoadmapOpts(0., 0., 0))
  gusto_check(ccall((:gusto_default_roadmap_opts, libgusto_hip), Cint, (Cint, Ref{GustoRoadmapOpts}), model_id, d), h, "default_roadmap_opts")
  o = GustoRoadmapOpts(inflate === nothing ? d[].inflate : inflate, pad === nothing ? d[].pad : pad, straight_first ? 1 : 0)
  gusto_check(ccall((:gusto_set_problems_roadmap, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GustoRoadmapOpts}),
                    h, Bq, K, x0, lo, hi, tf, o), h, "set_problems_roadmap")
  status, n_via, via, len = zeros(Cint, B), zeros(Cint, B), zeros(Cint, GUSTO_ROADMAP_MAX_VIA, B), zeros(B)
  banned, stage = zeros(Cint, GUSTO_ROADMAP_MAX_K, B), zeros(3)
  GC.@preserve status n_via via len banned stage begin
    rep = GustoRoadmapReport(pointer(status), pointer(n_via), pointer(via), pointer(len), pointer(banned), pointer(stage))
    gusto_check(ccall((:gusto_get_roadmap, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoRoadmapReport}), h, rep), h, "get_roadmap")
  end
  ms = Ref{Cdouble}(0.)
  gusto_check(ccall((:gusto_last_roadmap_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, ms), h, "last_roadmap_ms")
  (status = status, n_via = n_via, via = via, length = len, banned = banned, stage_ms = stage, ms = ms[])
end

# Every TOP is one planning QUERY, seeded by set_problems_roadmap! with K alternates, solved in one launch of Q K problems and
# answered with the best alternate that is converged and successful (gusto_select_best on the last true cost).  fallback_fan: the
# queries without a winner go through solve_SCP_multistart_batch!'s fan afterwards (true = gusto_default_fan).  Returns per query
# (winner, cost, source, status): the winning alternate (1-based; 0 = none qualified), its cost (Inf likewise), :roadmap, :fan or
# :none, and the roadmap status of the winning alternate's seed (of alternate 1 without a roadmap winner).  All TOPs share model, N
# and the environment.
function solve_SCP_roadmap_batch!(TOSs::Vector, TOPs::Vector; K=1, fallback_fan=nothing, straight_first=false, inflate=nothing, pad=nothing,
                                  max_iter=30, force=false, device=0)
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, Q = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N && T.PD.env === TOP0.PD.env, TOPs) ||
    error("solve_SCP_roadmap_batch!: all problems must share the model type, N and the environment")
  alg0 = SCPParam_GuSTO(model)
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail,
                      SCPParam(model, TOP0.fixed_final_time).convergence_threshold)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, Q * K, gusto_hist_cap(max_iter), device), href[], "create")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                    h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
  boxes, spheres = gusto_env_tables(TOP0.PD.env)
  gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                    h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat(first.(bounds)...), hcat(last.(bounds)...)
  tf = Float64[T.tf_guess for T in TOPs]
  info = set_problems_roadmap!(h, gusto_model_id(model), x0, lo, hi, tf; K=K, inflate=inflate, pad=pad, straight_first=straight_first)
  B = Q * K
  gusto_check(ccall((:gusto_solve, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, max_iter, force), h, "solve")
  X, U = zeros(n, N, B), zeros(m, N, B)
  gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
  its, conv, succ, stop = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
  gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}),
                    h, its, conv, succ, stop, C_NULL), h, "get_status")
  duals = zeros(n, B)
  gusto_check(ccall((:gusto_get_dual, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, duals), h, "get_dual")
  msec = Ref{Cdouble}(0.)
  ccall((:gusto_last_solve_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, msec)
  Hs = gusto_histories(h, B)
  gusto_check(ccall((:gusto_select_best, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cint}), h, K, C_NULL, C_NULL), h, "select_best")
  win, wp, best = zeros(Cint, Q), zeros(Cint, Q), zeros(Q)
  GC.@preserve win wp best begin
    rep = GustoBestReport(pointer(win), pointer(wp), C_NULL, pointer(best), C_NULL, C_NULL)
    gusto_check(ccall((:gusto_get_best, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoBestReport}), h, rep), h, "get_best")
  end
  result = Vector{Any}(undef, Q)
  for q in 1:Q
    j = win[q] >= 0 ? wp[q] + 1 : (q - 1) * K + 1
    SCPP = SCPProblem(TOPs[q])
    SCPP.param.alg = SCPParam_GuSTO(model)
    SCPS = SCPSolution(SCPP, Trajectory(X[:, :, j], U[:, :, j], TOPs[q].tf_guess))
    gusto_fill_solution!(SCPS, SCPP.param.alg, Hs, j, its[j], conv[j], succ[j], stop[j], duals[:, j])
    SCPS.total_time = msec[] / 1e3 / B
    SCPS.iter_elapsed_times = vcat(0., fill(SCPS.total_time / max(1, its[j]), its[j]))
    SCPP.param.obstacle_toggle_distance = SCPP.param.alg.Δ_vec[end] / 8 + model.clearance
    TOSs[q].traj, TOSs[q].SCPS = SCPS.traj, SCPS
    result[q] = (winner = win[q] + 1, cost = win[q] >= 0 ? best[q] : Inf, source = win[q] >= 0 ? :roadmap : :none, status = info.status[j])
  end
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  lost = findall(r -> r.winner == 0, result)
  if fallback_fan !== nothing && fallback_fan !== false && !isempty(lost)
    fan = fallback_fan === true ? nothing : fallback_fan
    again = solve_SCP_multistart_batch!(TOSs[lost], TOPs[lost]; fan=fan, policy=:all, max_iter=max_iter, force=force, device=device)
    for (i, q) in enumerate(lost)
      again[i][1] > 0 && (result[q] = (winner = again[i][1], cost = again[i][2], source = :fan, status = result[q].status))
    end
  end
  result
end

# ---- final-time search: per query the shortest final time whose solve is eligible (csrc/tfsearch.hip) --------------------------
# fixed_final_time = false is inert in the reference: Tf is a variable with the single row Tf >= 0.1 and every solve runs at the
# caller's guess.  The search runs around gusto_solve: K candidate final times per query and round, the bracket, the incumbent
# plans, the next candidates and their seeds kept on the device.  include/gusto_hip.h states the definitions.  Mirrors
# gusto.jl_amd/host.py: BatchSolver.tfsearch_begin / tfsearch_update / tfsearch_info, solve_SCP_min_time_batch.  This wrapper has
# not been run.
const GUSTO_TFSEARCH_SEED_LINE = 0
const GUSTO_TFSEARCH_SEED_INCUMBENT = 1
const GUSTO_TFSEARCH_NONE = 1
const GUSTO_TFSEARCH_DONE = 2
const GUSTO_TFSEARCH_FLOOR = 4
const GUSTO_TFSEARCH_NONMONOTONE = 8
struct GustoTfsearchOpts      # gusto_tfsearch_opts
  tf_lo::Cdouble; tf_hi::Cdouble
  rtol::Cdouble
  seed::Cint
end
mutable struct GustoTfsearchReport      # gusto_tfsearch_report
  status::Ptr{Cint}; round_found::Ptr{Cint}; n_eligible::Ptr{Cint}
  lo::Ptr{Cdouble}; hi::Ptr{Cdouble}; tf_best::Ptr{Cdouble}; J_best::Ptr{Cdouble}
  cand::Ptr{Cdouble}
  X::Ptr{Cdouble}; U::Ptr{Cdouble}
end

# Bq queries (columns of x0, lo, hi) x K candidate final times in [tf_lo[q], tf_hi[q]] become the B = Bq K problems of the handle
# h, problem (q - 1) K + j = candidate j of query q, each started from the straight line.  seed: :incumbent or :line.
function tfsearch_begin!(h::Ptr{Cvoid}, model_id::Integer, x0::Matrix{Float64}, lo::Matrix{Float64}, hi::Matrix{Float64},
                         tf_lo::Vector{Float64}, tf_hi::Vector{Float64}; K=8, rtol=0.01, seed=:incumbent)
  Bq = size(x0, 2)
  d = Ref(GustoTfsearchOpts(0., 0., 0., 0))
  gusto_check(ccall((:gusto_default_tfsearch_opts, libgusto_hip), Cint, (Cint, Ref{GustoTfsearchOpts}), model_id, d), h, "default_tfsearch_opts")
  o = GustoTfsearchOpts(d[].tf_lo, d[].tf_hi, rtol, seed == :line ? GUSTO_TFSEARCH_SEED_LINE : GUSTO_TFSEARCH_SEED_INCUMBENT)
  gusto_check(ccall((:gusto_tfsearch_begin, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GustoTfsearchOpts}),
                    h, Bq, K, x0, lo, hi, tf_lo, tf_hi, o), h, "tfsearch_begin")
  nothing
end

# The report of the search on h: (status, round_found, n_eligible, lo, hi, tf_best, J_best, cand [K, Bq], X [n, N, Bq], U [m, N, Bq],
# round, n_searching, ms)
function tfsearch_info(h::Ptr{Cvoid}, Bq::Integer, K::Integer, N::Integer, n::Integer, m::Integer)
  status, found, ne = zeros(Cint, Bq), zeros(Cint, Bq), zeros(Cint, Bq)
  lo, hi, tfb, Jb, cand = zeros(Bq), zeros(Bq), zeros(Bq), zeros(Bq), zeros(K, Bq)
  X, U = zeros(n, N, Bq), zeros(m, N, Bq)
  rd, ns = Ref{Cint}(0), Ref{Cint}(0)
  GC.@preserve status found ne lo hi tfb Jb cand X U begin
    rep = GustoTfsearchReport(pointer(status), pointer(found), pointer(ne), pointer(lo), pointer(hi), pointer(tfb), pointer(Jb),
                              pointer(cand), pointer(X), pointer(U))
    gusto_check(ccall((:gusto_get_tfsearch, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoTfsearchReport}, Ref{Cint}, Ref{Cint}), h, rep, rd, ns),
                h, "get_tfsearch")
  end
  ms = Ref{Cdouble}(0.)
  gusto_check(ccall((:gusto_last_tfsearch_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, ms), h, "last_tfsearch_ms")
  (status = status, round_found = found, n_eligible = ne, lo = lo, hi = hi, tf_best = tfb, J_best = Jb, cand = cand, X = X, U = U,
   round = Int(rd[]), n_searching = Int(ns[]), ms = ms[])
end

# After a solve of the round's problems: incumbents, brackets, status words, the next candidates and seeds; the problems of the
# queries that are done become inactive.  eligible: nothing (converged and successful) or a Bool / integer vector [B].  Returns
# the number of queries still searching.
function tfsearch_update!(h::Ptr{Cvoid}; eligible=nothing)
  el = eligible === nothing ? C_NULL : Cint.(eligible .!= 0)
  gusto_check(ccall((:gusto_tfsearch_update, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}), h, el), h, "tfsearch_update")
  ns = Ref{Cint}(0)
  gusto_check(ccall((:gusto_get_tfsearch, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cint}, Ref{Cint}), h, C_NULL, C_NULL, ns),
              h, "get_tfsearch")
  Int(ns[])
end

# Device pointers to the incumbents [n, N, Bq], [m, N, Bq] and tf_best [Bq]
function tfsearch_dev(h::Ptr{Cvoid})
  px, pu, pt = Ref{Ptr{Cdouble}}(C_NULL), Ref{Ptr{Cdouble}}(C_NULL), Ref{Ptr{Cdouble}}(C_NULL)
  gusto_check(ccall((:gusto_get_tfsearch_dev, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Ptr{Cdouble}}, Ref{Ptr{Cdouble}}, Ref{Ptr{Cdouble}}),
                    h, px, pu, pt), h, "get_tfsearch_dev")
  (X = px[], U = pu[], tf_best = pt[])
end

# Every TOP is one planning QUERY, answered with the shortest final time in [tf_lo, tf_hi] (numbers or one per query) whose solve
# is eligible: at most `rounds` rounds of K candidates.  eligible: nothing, or a function of (h, B) that returns the mask [B]
# after a round's solve.  Returns per query (tf, lo, hi, status, J); TOSs[q].traj is the incumbent with Tf = tf, TOSs[q].SCPS the
# solution of the solve that found it (without an incumbent: of the straight line's solve at tf_hi).  All TOPs share model, N and
# the environment.  TrajectoryOptimizationProblem(...; fixed_final_time=false) stays as inert as in the reference.
function solve_SCP_min_time_batch!(TOSs::Vector, TOPs::Vector, tf_lo, tf_hi; K=8, rounds=3, rtol=0.01, seed=:incumbent, eligible=nothing,
                                   max_iter=30, force=false, device=0)
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, Q = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N && T.PD.env === TOP0.PD.env, TOPs) ||
    error("solve_SCP_min_time_batch!: all problems must share the model type, N and the environment")
  alg0 = SCPParam_GuSTO(model)
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail,
                      SCPParam(model, TOP0.fixed_final_time).convergence_threshold)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, Q * K, gusto_hist_cap(max_iter), device), href[], "create")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                    h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
  boxes, spheres = gusto_env_tables(TOP0.PD.env)
  gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                    h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat(first.(bounds)...), hcat(last.(bounds)...)
  tlo = tf_lo isa Number ? fill(Float64(tf_lo), Q) : Float64.(tf_lo)
  thi = tf_hi isa Number ? fill(Float64(tf_hi), Q) : Float64.(tf_hi)
  tfsearch_begin!(h, gusto_model_id(model), x0, lo, hi, tlo, thi; K=K, rtol=rtol, seed=seed)
  B = Q * K
  info = tfsearch_info(h, Q, K, N, n, m)
  taken = falses(Q)
  for r in 0:rounds-1
    cand = info.cand
    gusto_check(ccall((:gusto_solve, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, max_iter, force), h, "solve")
    X, U = zeros(n, N, B), zeros(m, N, B)
    gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
    its, conv, succ, stop = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
    gusto_check(ccall((:gusto_get_status, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}),
                      h, its, conv, succ, stop, C_NULL), h, "get_status")
    duals = zeros(n, B)
    gusto_check(ccall((:gusto_get_dual, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, duals), h, "get_dual")
    msec = Ref{Cdouble}(0.)
    ccall((:gusto_last_solve_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, msec)
    Hs = gusto_histories(h, B)
    ok = eligible === nothing ? (conv .!= 0) .& (succ .!= 0) : Bool.(eligible(h, B) .!= 0)
    searching = tfsearch_update!(h; eligible = eligible === nothing ? nothing : ok)
    info = tfsearch_info(h, Q, K, N, n, m)
    for q in 1:Q
      j = 0
      if info.round_found[q] == r         # the incumbent of this round: the lowest candidate at tf_best that counts
        j = (q - 1) * K + findfirst(i -> ok[(q - 1) * K + i] && cand[i, q] == info.tf_best[q], 1:K)
      elseif !taken[q] && info.round_found[q] < 0
        j = q * K                         # (round 0, no incumbent: the line at tf_hi)
      end
      j == 0 && continue
      taken[q] = true
      SCPP = SCPProblem(TOPs[q])
      SCPP.param.alg = SCPParam_GuSTO(model)
      SCPS = SCPSolution(SCPP, Trajectory(X[:, :, j], U[:, :, j], cand[(j - 1) % K + 1, q]))
      gusto_fill_solution!(SCPS, SCPP.param.alg, Hs, j, its[j], conv[j], succ[j], stop[j], duals[:, j])
      SCPS.total_time = msec[] / 1e3 / B
      SCPS.iter_elapsed_times = vcat(0., fill(SCPS.total_time / max(1, its[j]), its[j]))
      SCPP.param.obstacle_toggle_distance = SCPP.param.alg.Δ_vec[end] / 8 + model.clearance
      TOSs[q].traj, TOSs[q].SCPS = SCPS.traj, SCPS
    end
    searching == 0 && break
  end
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  [(tf = info.tf_best[q], lo = info.lo[q], hi = info.hi[q], status = Int(info.status[q]), J = info.J_best[q]) for q in 1:Q]
end

# ---- goal timeline: the goals of a query before its final time, flown as legs and joined on the device (csrc/legs.hip) ---------
# A GoalSet is keyed by time, but every goal row function hard-codes knot N: a goal before the final time is carried and ignored
# by the solve.  The timeline runs around gusto_solve: every goal interval is a leg, an ordinary problem from the previous
# junction to that goal in the time between the two; the report and the joined trajectories stay on the device.
# include/gusto_hip.h states the definitions.  Mirrors gusto.jl_amd/host.py: BatchSolver.legs_begin / legs_advance / legs_info,
# solve_SCP_timeline_batch.  This wrapper has not been run.
const GUSTO_LEGS_AUTO = 0
const GUSTO_LEGS_SEQUENTIAL = 1
const GUSTO_LEGS_PARALLEL = 2
const GUSTO_LEGS_FLYING = 1
const GUSTO_LEGS_DONE = 2
const GUSTO_LEGS_FAILED = 4
struct GustoLegsOpts      # gusto_legs_opts
  mode::Cint
end
mutable struct GustoLegsReport      # gusto_legs_report
  status::Ptr{Cint}; failed_leg::Ptr{Cint}; n_done::Ptr{Cint}
  J_total::Ptr{Cdouble}
  iterations::Ptr{Cint}; converged::Ptr{Cint}; successful::Ptr{Cint}; stop_reason::Ptr{Cint}
  J::Ptr{Cdouble}; gap::Ptr{Cdouble}; arrive::Ptr{Cdouble}
  X::Ptr{Cdouble}; U::Ptr{Cdouble}; t::Ptr{Cdouble}
end

# every goal of the GoalSet with 0 < t_guess <= tf_guess, grouped by time: [(T, lo, hi)] in the order of time, lo / hi by the rules
# of gusto_goal_bounds at that time.  A final time without a goal is an error.
function gusto_timeline_of(TOP)
  n, tf = TOP.PD.model.x_dim, TOP.tf_guess
  times = sort(unique([t for t in keys(TOP.PD.goal_set.goals) if 0 < t <= tf]))
  (isempty(times) || times[end] != tf) && error("gusto_timeline_of: no goal at the final time tf_guess")
  [(T, gusto_goal_bounds(TOP.PD.goal_set, n, T)...) for T in times]
end

# Bq queries (columns of x0) with L goals each -- lo, hi [n, L, Bq] at the times T [L, Bq], n_legs [Bq] of them per query -- are
# flown as legs on the handle h.  mode: :auto, :sequential (B = Bq, problem q is the query's current leg) or :parallel (B = Bq L,
# problem (q - 1) L + l = leg l of query q; every goal before the last must pin every coordinate).
function legs_begin!(h::Ptr{Cvoid}, model_id::Integer, x0::Matrix{Float64}, lo::Array{Float64,3}, hi::Array{Float64,3}, T::Matrix{Float64};
                     n_legs=nothing, mode=:auto)
  Bq, L = size(x0, 2), size(T, 1)
  d = Ref(GustoLegsOpts(0))
  gusto_check(ccall((:gusto_default_legs_opts, libgusto_hip), Cint, (Cint, Ref{GustoLegsOpts}), model_id, d), h, "default_legs_opts")
  o = GustoLegsOpts(mode == :sequential ? GUSTO_LEGS_SEQUENTIAL : mode == :parallel ? GUSTO_LEGS_PARALLEL : d[].mode)
  nl = n_legs === nothing ? C_NULL : Cint.(n_legs)
  gusto_check(ccall((:gusto_legs_begin, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{GustoLegsOpts}),
                    h, Bq, L, nl, x0, lo, hi, T, o), h, "legs_begin")
  nothing
end

# After a solve: the solved legs into the joined buffers and the report, the next legs' seeds; the problems of the finished
# queries become inactive.  eligible: nothing (converged and successful) or a Bool / integer vector [B].  Returns the number of
# queries still flying.
function legs_advance!(h::Ptr{Cvoid}; eligible=nothing)
  el = eligible === nothing ? C_NULL : Cint.(eligible .!= 0)
  gusto_check(ccall((:gusto_legs_advance, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}), h, el), h, "legs_advance")
  nf = Ref{Cint}(0)
  gusto_check(ccall((:gusto_get_legs, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cint}, Ref{Cint}), h, C_NULL, C_NULL, nf), h, "get_legs")
  Int(nf[])
end

# The report of the timeline on h: per query status, failed_leg, n_done, J_total; per leg [L, Bq] iterations, converged,
# successful, stop_reason, J, gap, arrive; the joined X [n, Nj, Bq], U [m, Nj, Bq], t [Nj, Bq] with Nj = L (N - 1) + 1; round,
# n_flying and the GPU time of the last begin or advance
function legs_info(h::Ptr{Cvoid}, Bq::Integer, L::Integer, N::Integer, n::Integer, m::Integer)
  Nj = L * (N - 1) + 1
  status, failed, ndone, Jt = zeros(Cint, Bq), zeros(Cint, Bq), zeros(Cint, Bq), zeros(Bq)
  its, conv, succ, stop = zeros(Cint, L, Bq), zeros(Cint, L, Bq), zeros(Cint, L, Bq), zeros(Cint, L, Bq)
  J, gap, arrive = zeros(L, Bq), zeros(L, Bq), zeros(L, Bq)
  X, U, t = zeros(n, Nj, Bq), zeros(m, Nj, Bq), zeros(Nj, Bq)
  rd, nf = Ref{Cint}(0), Ref{Cint}(0)
  GC.@preserve status failed ndone Jt its conv succ stop J gap arrive X U t begin
    rep = GustoLegsReport(pointer(status), pointer(failed), pointer(ndone), pointer(Jt), pointer(its), pointer(conv), pointer(succ),
                          pointer(stop), pointer(J), pointer(gap), pointer(arrive), pointer(X), pointer(U), pointer(t))
    gusto_check(ccall((:gusto_get_legs, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoLegsReport}, Ref{Cint}, Ref{Cint}), h, rep, rd, nf), h, "get_legs")
  end
  ms = Ref{Cdouble}(0.)
  gusto_check(ccall((:gusto_last_legs_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, ms), h, "last_legs_ms")
  (status = status, failed_leg = failed, n_done = ndone, J_total = Jt, iterations = its, converged = conv, successful = succ,
   stop_reason = stop, J = J, gap = gap, arrive = arrive, X = X, U = U, t = t, round = Int(rd[]), n_flying = Int(nf[]), ms = ms[])
end

# Device pointers to the joined X [n, Nj, Bq], U [m, Nj, Bq] and t [Nj, Bq]
function legs_dev(h::Ptr{Cvoid})
  px, pu, pt = Ref{Ptr{Cdouble}}(C_NULL), Ref{Ptr{Cdouble}}(C_NULL), Ref{Ptr{Cdouble}}(C_NULL)
  gusto_check(ccall((:gusto_get_legs_dev, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Ptr{Cdouble}}, Ref{Ptr{Cdouble}}, Ref{Ptr{Cdouble}}),
                    h, px, pu, pt), h, "get_legs_dev")
  (X = px[], U = pu[], t = pt[])
end

# Every TOP is one planning QUERY whose GoalSet is flown as a timeline: every goal time in (0, tf_guess] ends a leg.  mode as
# legs_begin!.  Returns per query (status, failed_leg, n_done, J_total, T, gap, arrive); TOSs[q].traj is the joined trajectory with
# Tf the last goal's time; its knot times are the `t` of the returned tuple.  All TOPs share model, N and the environment.  solve_SCP! keeps ignoring the goals before tf_guess, as the reference does.
function solve_SCP_timeline_batch!(TOSs::Vector, TOPs::Vector; mode=:auto, max_iter=30, force=false, device=0)
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, Q = model.x_dim, model.u_dim, length(TOPs)
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N && T.PD.env === TOP0.PD.env, TOPs) ||
    error("solve_SCP_timeline_batch!: all problems must share the model type, N and the environment")
  lines = [gusto_timeline_of(T) for T in TOPs]
  nl = length.(lines); L = maximum(nl)
  T, lo, hi = zeros(L, Q), fill(-Inf, n, L, Q), fill(Inf, n, L, Q)
  for q in 1:Q, (l, (t, a, b)) in enumerate(lines[q])
    T[l, q] = t; lo[:, l, q] = a; hi[:, l, q] = b
  end
  alg0 = SCPParam_GuSTO(model)
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail,
                      SCPParam(model, TOP0.fixed_final_time).convergence_threshold)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, Q * L, gusto_hist_cap(max_iter), device), href[], "create")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                    h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
  boxes, spheres = gusto_env_tables(TOP0.PD.env)
  gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                    h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  legs_begin!(h, gusto_model_id(model), x0, lo, hi, T; n_legs=nl, mode=mode)
  flying = Q
  while flying > 0
    gusto_check(ccall((:gusto_solve, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, max_iter, force), h, "solve")
    flying = legs_advance!(h)
  end
  info = legs_info(h, Q, L, N, n, m)
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  for q in 1:Q
    Nq = nl[q] * (N - 1) + 1
    TOSs[q].traj = Trajectory(info.X[:, 1:Nq, q], info.U[:, 1:Nq, q], T[nl[q], q])
  end
  [(status = Int(info.status[q]), failed_leg = Int(info.failed_leg[q]), n_done = Int(info.n_done[q]), J_total = info.J_total[q],
    T = T[1:nl[q], q], t = info.t[1:nl[q] * (N - 1) + 1, q], gap = info.gap[1:nl[q], q], arrive = info.arrive[1:nl[q], q]) for q in 1:Q]
end

# ---- fleet coordination (gusto_fleet_schedule / gusto_fleet_separation, csrc/fleet.hip) ---------------------------------------
# R consecutive problems of the handle are the robots of one fleet; every robot keeps its solved path and departs by the smallest
# candidate delay that keeps it `margin` away from every robot placed before it (include/gusto_hip.h states the definitions, the
# reference has no counterpart).  The call sequences are those of gusto.jl_amd/_capi.py and host.py.  This wrapper has not been run.
const GUSTO_FLEET_NO_PLAN = 0
const GUSTO_FLEET_SCHEDULED = 1
const GUSTO_FLEET_BLOCKED = 2
struct GustoFleetOpts      # gusto_fleet_opts
  dt_clock::Cdouble; margin::Cdouble
  n_delays::Cint; delay_stride::Cint; clock_cap::Cint; components::Cint; prune::Cint
end
mutable struct GustoFleetReport      # gusto_fleet_report
  status::Ptr{Cint}; delay_steps::Ptr{Cint}
  delay::Ptr{Cdouble}
  blocker::Ptr{Cint}
  min_sep::Ptr{Cdouble}
  partner::Ptr{Cint}; step::Ptr{Cint}
  pair_min_sep::Ptr{Cdouble}
  pair_step::Ptr{Cint}
  n_scheduled::Ptr{Cint}; n_blocked::Ptr{Cint}; n_conflicts::Ptr{Cint}
  fleet_min_sep::Ptr{Cdouble}
  makespan_steps::Ptr{Cint}
  stage_ms::Ptr{Cdouble}
end

# the library's defaults for the model, with the keywords over them
function gusto_fleet_opts(model_id::Integer; margin=nothing, dt_clock=nothing, n_delays=nothing, delay_stride=nothing, clock_cap=nothing,
                          components=nothing)
  d = Ref(GustoFleetOpts(0., 0., 0, 0, 0, 0, 0))
  gusto_check(ccall((:gusto_default_fleet_opts, libgusto_hip), Cint, (Cint, Ref{GustoFleetOpts}), model_id, d), C_NULL, "default_fleet_opts")
  pick(v, dflt) = v === nothing ? dflt : v
  GustoFleetOpts(pick(dt_clock, d[].dt_clock), pick(margin, d[].margin), pick(n_delays, d[].n_delays), pick(delay_stride, d[].delay_stride),
                 pick(clock_cap, d[].clock_cap), pick(components, d[].components), d[].prune)
end

# The report of the last fleet call on h, B = F R robots: per robot status, delay_steps, delay, blocker, min_sep, partner, step; per
# pair [R, R, F] pair_min_sep, pair_step; per fleet n_scheduled, n_blocked, n_conflicts, fleet_min_sep, makespan_steps; stage_ms
function fleet_info(h::Ptr{Cvoid})
  Fr, Rr = Ref{Cint}(0), Ref{Cint}(0)
  gusto_check(ccall((:gusto_get_fleet, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), h, C_NULL, Fr, Rr), h, "get_fleet")
  F, R = Int(Fr[]), Int(Rr[]); B = F * R
  status, steps, blocker, partner, step = zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B), zeros(Cint, B)
  delay, min_sep, pair_sep, pair_step = zeros(B), zeros(B), zeros(R, R, F), zeros(Cint, R, R, F)
  ns, nb, nc, span, fsep, ms = zeros(Cint, F), zeros(Cint, F), zeros(Cint, F), zeros(Cint, F), zeros(F), zeros(3)
  GC.@preserve status steps blocker partner step delay min_sep pair_sep pair_step ns nb nc span fsep ms begin
    rep = GustoFleetReport(pointer(status), pointer(steps), pointer(delay), pointer(blocker), pointer(min_sep), pointer(partner),
                           pointer(step), pointer(pair_sep), pointer(pair_step), pointer(ns), pointer(nb), pointer(nc), pointer(fsep),
                           pointer(span), pointer(ms))
    gusto_check(ccall((:gusto_get_fleet, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoFleetReport}, Ptr{Cint}, Ptr{Cint}), h, rep, C_NULL, C_NULL),
                h, "get_fleet")
  end
  total = Ref{Cdouble}(0.)
  gusto_check(ccall((:gusto_last_fleet_ms, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), h, total), h, "last_fleet_ms")
  (status = status, delay_steps = steps, delay = delay, blocker = blocker, min_sep = min_sep, partner = partner, step = step,
   pair_min_sep = pair_sep, pair_step = pair_step, n_scheduled = ns, n_blocked = nb, n_conflicts = nc, fleet_min_sep = fsep,
   makespan_steps = span, stage_ms = ms, ms = total[], F = F, R = R)
end

# After gusto_interpolate: the departure schedule of fleets of R robots.  order: nothing (index order) or [R, F], 0-based robot
# indices in placement order; eligible: nothing (converged and successful) or a Bool / integer vector [B].  Returns fleet_info.
function fleet_schedule!(h::Ptr{Cvoid}, R::Integer, opts::GustoFleetOpts; order=nothing, eligible=nothing)
  od = order === nothing ? C_NULL : Cint.(vec(order))
  el = eligible === nothing ? C_NULL : Cint.(eligible .!= 0)
  gusto_check(ccall((:gusto_fleet_schedule, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cint}, Ref{GustoFleetOpts}), h, R, od, el, opts),
              h, "fleet_schedule")
  fleet_info(h)
end

# The pairwise separation report for the last schedule's shifts (delay_steps = nothing) or for delay_steps [B] in clock steps,
# -1 = the robot never departs.  Returns fleet_info.
function fleet_separation!(h::Ptr{Cvoid}, R::Integer, opts::GustoFleetOpts; delay_steps=nothing)
  ds = delay_steps === nothing ? C_NULL : Cint.(delay_steps)
  gusto_check(ccall((:gusto_fleet_separation, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}, Ref{GustoFleetOpts}), h, R, ds, opts),
              h, "fleet_separation")
  fleet_info(h)
end

# The clock tracks of the last fleet call: (J [B], Q [WS, J_max, B])
function fleet_tracks(h::Ptr{Cvoid}, B::Integer, ws::Integer)
  jm = Ref{Cint}(0)
  gusto_check(ccall((:gusto_get_fleet_tracks, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cdouble}, Ref{Cint}), h, C_NULL, C_NULL, jm), h, "get_fleet_tracks")
  J, Q = zeros(Cint, B), zeros(ws, Int(jm[]), B)
  gusto_check(ccall((:gusto_get_fleet_tracks, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}), h, J, Q, C_NULL), h, "get_fleet_tracks")
  (J, Q)
end

# Every TOP is one ROBOT, R consecutive TOPs one fleet: solve, interpolate, fleet_schedule!, fleet_separation!.  All TOPs share
# model, N and the environment; whether a robot can hold at its start and park at its goal is the caller's business.  The parking
# keep-outs of the Python driver (host.fleet_park_spheres) are not built here: pass environments that hold them.  Returns
# fleet_info; TOSs[q].traj is robot q's trajectory, its departure delay is the report's delay[q].
function solve_SCP_fleet_batch!(TOSs::Vector, TOPs::Vector, R::Integer; margin=nothing, order=nothing, fleet_opts=(;), max_iter=30,
                                force=false, device=0)
  TOP0 = TOPs[1]; model, N = TOP0.PD.model, TOP0.N
  n, m, Q = model.x_dim, model.u_dim, length(TOPs)
  (R >= 1 && Q % R == 0) || error("solve_SCP_fleet_batch!: R must divide the number of problems")
  all(T -> typeof(T.PD.model) == typeof(model) && T.N == N && T.PD.env === TOP0.PD.env, TOPs) ||
    error("solve_SCP_fleet_batch!: all problems must share the model type, N and the environment")
  alg0 = SCPParam_GuSTO(model)
  sp = GustoScpParams(alg0.Δ0, alg0.ω0, alg0.ω_max, alg0.ε, alg0.ρ0, alg0.ρ1, alg0.β_succ, alg0.β_fail, alg0.γ_fail,
                      SCPParam(model, TOP0.fixed_final_time).convergence_threshold)
  href = Ref{Ptr{Cvoid}}(C_NULL)
  gusto_check(ccall((:gusto_create, libgusto_hip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint),
                    href, gusto_model_id(model), N, Q, gusto_hist_cap(max_iter), device), href[], "create")
  h = href[]
  gusto_check(ccall((:gusto_set_params, libgusto_hip), Cint, (Ptr{Cvoid}, Ref{GustoScpParams}, Ref{GustoModelParams}),
                    h, sp, gusto_model_params(TOP0.PD.robot, model)), h, "set_params")
  boxes, spheres = gusto_env_tables(TOP0.PD.env)
  gusto_check(ccall((:gusto_set_env, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                    h, length(boxes) ÷ 6, boxes, length(spheres) ÷ 4, spheres), h, "set_env")
  x0 = hcat((Float64.(T.PD.x_init) for T in TOPs)...)
  bounds = [gusto_goal_bounds(T.PD.goal_set, n, T.tf_guess) for T in TOPs]
  lo, hi = hcat((b[1] for b in bounds)...), hcat((b[2] for b in bounds)...)
  tf = Float64[T.tf_guess for T in TOPs]
  gusto_check(ccall((:gusto_set_problems, libgusto_hip), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    h, Q, x0, lo, hi, tf, C_NULL, C_NULL), h, "set_problems")
  gusto_check(ccall((:gusto_solve, libgusto_hip), Cint, (Ptr{Cvoid}, Cint, Cint), h, max_iter, force), h, "solve")
  X, U = zeros(n, N, Q), zeros(m, N, Q)
  gusto_check(ccall((:gusto_get_traj, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, X, U), h, "get_traj")
  gusto_check(ccall((:gusto_interpolate, libgusto_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Ptr{Cint}),
                    h, C_NULL, C_NULL, C_NULL, C_NULL), h, "interpolate")
  o = gusto_fleet_opts(gusto_model_id(model); margin=margin, fleet_opts...)
  fleet_schedule!(h, R, o; order=order)
  info = fleet_separation!(h, R, o)
  ccall((:gusto_destroy, libgusto_hip), Cint, (Ptr{Cvoid},), h)
  for q in 1:Q
    TOSs[q].traj = Trajectory(X[:, :, q], U[:, :, q], tf[q])
  end
  info
end
