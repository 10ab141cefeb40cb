# AGPLDeviceExt.jl -- package extension routing AugmentedGPLikelihoods.jl's operator surface to libagpl.so
# (include/agpl.h) for AMDGPU.jl device arrays.  Drop it into the package's `ext/` directory with
#
#     [weakdeps]   AMDGPU = "21141c5a-9bdb-4563-92ae-f87d6854732e"      (KernelFunctions, whose kernel types the plan constructor
#                                                                         dispatches on, is a dependency of the package's examples)
#     [extensions] AGPLDeviceExt = "AMDGPU"
#
# Nothing in the package's own methods changes: these are additional methods of the SAME generic functions
# (src/generic.jl:5-72, src/likelihoods/*.jl) dispatching on ROCArray arguments, so every existing call site
# (examples/*/script.jl, an SVGP loop over ApproximateGPs) keeps its code and gets the device path by passing
# device arrays.  One `ccall` per operator; status codes become the exception types the reference throws.
#
# STATUS: written against include/agpl.h v110 (the plan API), not executed -- the build image has no `julia` (SURVEY.md F6).  The
# executed twin is the Python host (augmentedgplikelihoods.jl_amd/operators.py, sparse.py): same entry point per
# operator, same argument order.  tests/test_julia_artifacts.py checks that every `ccall` below names an exported
# symbol with the right number of arguments.
module AGPLDeviceExt

using AugmentedGPLikelihoods
using AMDGPU
using Random
using LinearAlgebra
using Distributions: Normal, mean, var
using TupleVectors: TupleVector
using ArraysOfArrays: flatview
using KernelFunctions: SqExponentialKernel, ExponentialKernel, Matern32Kernel, Matern52Kernel, RationalQuadraticKernel

using AugmentedGPLikelihoods: AbstractLikelihood, BernoulliLikelihood, NegativeBinomialLikelihood, NBParamFailure,
    StudentTLikelihood, CategoricalLikelihood, PoissonLikelihood, LaplaceLikelihood,
    HeteroscedasticGaussianLikelihood, LogisticLink, LogisticSoftMaxLink, BijectiveSimplexLink, ScaledLogistic,
    InvScaledLogistic, nlatent
import AugmentedGPLikelihoods: aux_sample!, aux_posterior!, auglik_potential, auglik_precision,
    auglik_potential_and_precision, expected_auglik_potential, expected_auglik_precision,
    expected_auglik_potential_and_precision, logtilt, aug_loglik, expected_logtilt, expected_aug_loglik, aux_kldivergence

const libagpl = get(ENV, "AGPL_LIB", "libagpl.so")
const libagpl_predictive = get(ENV, "AGPL_PREDICTIVE_LIB", "libagpl_predictive.so")   # include/agpl_predictive.h: p(y*) under q(f)
const libagpl_se = get(ENV, "AGPL_SE_LIB", "libagpl_se.so")   # include/agpl_se.h: SE plans from raw inputs, prediction
const libagpl_chain = get(ENV, "AGPL_CHAIN_LIB", "libagpl_chain.so")   # include/agpl_chain.h: a chain of inducing draws at new inputs
const libagpl_kernels = get(ENV, "AGPL_KERNELS_LIB", "libagpl_kernels.so")   # include/agpl_kernels.h: plans from raw inputs, Matern / RQ kernels
const libagpl_joint = get(ENV, "AGPL_JOINT_LIB", "libagpl_joint.so")   # include/agpl_joint.h: the posterior covariance between new inputs
const libagpl_inducing = get(ENV, "AGPL_INDUCING_LIB", "libagpl_inducing.so")   # include/agpl_inducing.h: k-means inducing inputs
const libagpl_greedy = get(ENV, "AGPL_GREEDY_LIB", "libagpl_greedy.so")   # include/agpl_greedy.h: greedy conditional-variance inducing inputs
const libagpl_loo = get(ENV, "AGPL_LOO_LIB", "libagpl_loo.so")   # include/agpl_loo.h: the leave-one-out cavity at the training points
const libagpl_grad = get(ENV, "AGPL_GRAD_LIB", "libagpl_grad.so")   # include/agpl_grad.h: the posterior of the gradient of f at new inputs
const libagpl_quantile = get(ENV, "AGPL_QUANTILE_LIB", "libagpl_quantile.so")   # include/agpl_quantile.h: the predictive distribution function of y and its quantiles
const libagpl_likgrad = get(ENV, "AGPL_LIKGRAD_LIB", "libagpl_likgrad.so")   # include/agpl_likgrad.h: E_q log p(y | f) and its gradient for the likelihood's parameters

# ------------------------------------------------------------------------------------------------ descriptor
# mirrors agpl_lik_desc; logtheta is a HOST pointer that must stay alive across the call (GC.@preserve below)
struct LikDesc
    kind::Int32
    nlatent::Int32
    p::NTuple{4,Float64}
    logtheta::Ptr{Float64}
end
const P0 = (0.0, 0.0, 0.0, 0.0)

# (descriptor, object to GC.@preserve) per likelihood family = per file of src/likelihoods/
desc(::BernoulliLikelihood{<:LogisticLink}) = (LikDesc(0, 1, P0, C_NULL), nothing)
function desc(l::NegativeBinomialLikelihood{<:NBParamFailure})
    return (LikDesc(1, 1, (Float64(l.params.failures), 0.0, 0.0, 0.0), C_NULL), nothing)
end
desc(l::StudentTLikelihood) = (LikDesc(2, 1, (Float64(l.ν), Float64(l.σ), 0.0, 0.0), C_NULL), nothing)
function desc(l::CategoricalLikelihood{<:LogisticSoftMaxLink})        # categorical.jl:9-10, nlatent = K
    θ = convert(Vector{Float64}, l.invlink.logθ)
    return (LikDesc(3, length(θ), P0, pointer(θ)), θ)
end
function desc(l::CategoricalLikelihood{<:BijectiveSimplexLink{<:LogisticSoftMaxLink}})   # nlatent = K - 1
    θ = convert(Vector{Float64}, l.invlink.link.logθ)
    return (LikDesc(4, length(θ) - 1, P0, pointer(θ)), θ)
end
desc(l::PoissonLikelihood{<:ScaledLogistic}) = (LikDesc(5, 1, (Float64(l.invlink.λ), 0.0, 0.0, 0.0), C_NULL), nothing)
desc(l::LaplaceLikelihood) = (LikDesc(6, 1, (Float64(l.β), 0.0, 0.0, 0.0), C_NULL), nothing)
function desc(l::HeteroscedasticGaussianLikelihood{<:InvScaledLogistic})
    return (LikDesc(7, 2, (Float64(l.invlink.λ), 0.0, 0.0, 0.0), C_NULL), nothing)
end

# Binomial with a trial count per point (AGPL_LIK_BINOMIAL_N; no type in the reference package): y is Int32 [2, N], (successes; trials)
struct BinomialTrials end
desc(::BinomialTrials) = (LikDesc(11, 1, P0, C_NULL), nothing)

# ------------------------------------------------------------------------------------------------ context
# replaces GLOBAL_RNG / the `rng` argument (src/generic.jl:1-3): Philox key = seed, `sweep` = draw counter
mutable struct Ctx
    h::Ptr{Cvoid}
    sweep::UInt32
end

function check(h::Ptr{Cvoid}, rc::Integer)
    rc == 0 && return nothing
    msg = h == C_NULL ? "libagpl status $rc" :
          unsafe_string(ccall((:agpl_last_error, libagpl), Cstring, (Ptr{Cvoid},), h))
    rc == -1 && throw(ArgumentError(msg))       # negativemultinomial.jl:17-22
    rc == -2 && throw(DomainError(NaN, msg))     # polyagamma.jl:175
    rc == -5 && throw(PosDefException(0))        # the M x M Cholesky
    rc == -6 && throw(OutOfMemoryError())
    return error(msg)                            # categorical.jl:165-170, polyagamma.jl:100-104
end

function Ctx(dev::Integer=0; seed::Integer=rand(UInt64))
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(C_NULL, ccall((:agpl_ctx_create, libagpl), Int32, (Ref{Ptr{Cvoid}}, Int32, UInt64), r, dev, seed))
    c = Ctx(r[], 0)
    finalizer(c -> ccall((:agpl_ctx_destroy, libagpl), Int32, (Ptr{Cvoid},), c.h), c)
    return c
end

const CTX = Ref{Ctx}()
ctx() = isassigned(CTX) ? CTX[] : (CTX[] = Ctx())
function next_sweep!(c::Ctx)
    s = c.sweep
    c.sweep += one(UInt32)
    return s
end
synchronize(c::Ctx=ctx()) = check(c.h, ccall((:agpl_ctx_synchronize, libagpl), Int32, (Ptr{Cvoid},), c.h))
"Global index of this rank's first point: per-point Philox streams are keyed on offset + i (N sharded over ranks)."
function set_point_offset!(c::Ctx, i0::Integer)
    return check(c.h, ccall((:agpl_ctx_set_point_offset, libagpl), Int32, (Ptr{Cvoid}, Int64), c.h, i0))
end

dptr(a::ROCArray) = Ptr{Cvoid}(UInt(pointer(a)))
dptr(::Nothing) = Ptr{Cvoid}(0)
field(tv, s::Symbol) = hasproperty(tv, s) ? getproperty(tv, s) : nothing
flat(a) = a isa ROCArray ? a : flatview(a)      # nestedview([L, N]) containers (categorical.jl:52-70) -> flat [L, N]
npoints(lik, f) = length(flat(f)) ÷ nlatent(lik)

# ------------------------------------------------------------------------------------------------ device marginals
"""
    DeviceNormals(mean, var)

What the device `marginals` returns in place of the `Vector{Normal}` the reference's methods receive
(`bernoulli.jl:17-25`): the same q(f_i) = N(mean_i, var_i) as two device arrays ([N], or [L, N] column-major for
multi-latent likelihoods).  `DeviceNormals(qf::AbstractVector{<:Normal})` uploads a host vector, so a call site
that still computes `marginals(...)` on the CPU keeps working.
"""
struct DeviceNormals{T<:ROCArray{Float64}}
    mean::T
    var::T
end
DeviceNormals(qf::AbstractVector{<:Normal}) = DeviceNormals(ROCArray(mean.(qf)), ROCArray(var.(qf)))
Base.length(q::DeviceNormals) = length(q.mean)

# ------------------------------------------------------------------------------------------------ Gibbs half
# aux_sample!(rng, Ω, lik, y, f)  src/generic.jl:5-12  ->  agpl_aux_sample.  The rng argument is accepted for
# signature compatibility; the draws come from the context's Philox streams (seed, point, sweep).
function aux_sample!(::AbstractRNG, Ω::TupleVector, lik::AbstractLikelihood, y::ROCArray, f::ROCArray{Float64})
    c = ctx()
    d, keep = desc(lik)
    ω, n = flat(Ω.ω), field(Ω, :n)
    n = n === nothing ? nothing : flat(n)
    GC.@preserve keep check(c.h, ccall((:agpl_aux_sample, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, UInt32, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, d, npoints(lik, f), dptr(y), dptr(f), dptr(ω), dptr(n), next_sweep!(c), C_NULL, C_NULL))
    return Ω                                      # mutated in place and returned, as generic.jl:11
end

# auglik_potential / auglik_precision / _and_precision  (generic.jl:64-66; bernoulli.jl:27-33 ...)  -> agpl_potential_precision
function auglik_potential_and_precision(lik::AbstractLikelihood, Ω::TupleVector, y::ROCArray, f=nothing)
    c = ctx()
    d, keep = desc(lik)
    L = nlatent(lik)
    N = length(y) ÷ (lik isa CategoricalLikelihood ? L : 1)
    β = ROCArray{Float64}(undef, N, L)            # L contiguous vectors of N (utils.jl:24)
    γ = similar(β)
    n = field(Ω, :n)
    GC.@preserve keep check(c.h, ccall((:agpl_potential_precision, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, d, N, dptr(y), dptr(flat(Ω.ω)), dptr(n === nothing ? nothing : flat(n)),
        dptr(f === nothing ? nothing : flat(f)), dptr(β), dptr(γ)))
    return ntuple(l -> view(β, :, l), L), ntuple(l -> view(γ, :, l), L)
end
auglik_potential(lik::AbstractLikelihood, Ω::TupleVector, y::ROCArray, f=nothing) =
    first(auglik_potential_and_precision(lik, Ω, y, f))
auglik_precision(lik::AbstractLikelihood, Ω::TupleVector, y::ROCArray, f=nothing) =
    last(auglik_potential_and_precision(lik, Ω, y, f))

# ------------------------------------------------------------------------------------------------ CAVI half
# which fields of only(qΩ.inds) are out1 / out2 / out3 of agpl_aux_posterior (include/agpl.h)
out1(lik, φ) = lik isa StudentTLikelihood ? φ.β : lik isa LaplaceLikelihood ? φ.μ : φ.c
out2(φ) = hasproperty(φ, :p) ? φ.p : field(φ, :λ)
out3(φ) = field(φ, :ψ)

# aux_posterior!(qΩ, lik, y, qf)  bernoulli.jl:17-25, negativebinomial.jl:24-33, studentt.jl:50-58,
# categorical.jl:80-110, poisson.jl:30-39, laplace.jl:44-52, heteroscedasticgaussian.jl:34-46 -> agpl_aux_posterior
function aux_posterior!(qΩ, lik::AbstractLikelihood, y::ROCArray, qf::DeviceNormals)
    c = ctx()
    d, keep = desc(lik)
    φ = only(qΩ.inds)
    o2, o3 = out2(φ), out3(φ)
    GC.@preserve keep check(c.h, ccall((:agpl_aux_posterior, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, d, 1 #= AGPL_F64 =#, npoints(lik, qf.mean), dptr(y), dptr(qf.mean), dptr(qf.var),
        dptr(flat(out1(lik, φ))), dptr(o2 === nothing ? nothing : flat(o2)), dptr(o3)))
    hasproperty(φ, :y) && copyto!(flat(φ.y), y)   # negativebinomial.jl:28, poisson.jl:35, categorical.jl:84
    return qΩ
end
# the reference's own argument type: a host Vector{Normal} is uploaded and routed to the method above
aux_posterior!(qΩ, lik::AbstractLikelihood, y::ROCArray, qf::AbstractVector{<:Normal}) =
    aux_posterior!(qΩ, lik, y, DeviceNormals(qf))

# expected_auglik_potential / _precision / _and_precision  (generic.jl:68-72; bernoulli.jl:35-45 ...)
# f = DeviceNormals of the latent(s) for the heteroscedastic likelihood (mu_g), else unused
function expected_auglik_potential_and_precision(lik::AbstractLikelihood, qΩ, y::ROCArray, f=nothing)
    c = ctx()
    d, keep = desc(lik)
    φ = only(qΩ.inds)
    L = nlatent(lik)
    N = length(y) ÷ (lik isa CategoricalLikelihood ? L : 1)
    β = ROCArray{Float64}(undef, N, L)
    γ = similar(β)
    o2 = out2(φ)
    μg = f isa DeviceNormals ? f.mean : nothing
    GC.@preserve keep check(c.h, ccall((:agpl_expected_potential_precision, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, d, 1, N, dptr(y), dptr(flat(out1(lik, φ))), dptr(o2 === nothing ? nothing : flat(o2)), dptr(μg),
        dptr(β), dptr(γ)))
    return ntuple(l -> view(β, :, l), L), ntuple(l -> view(γ, :, l), L)
end
expected_auglik_potential(lik::AbstractLikelihood, qΩ, y::ROCArray, f=nothing) =
    first(expected_auglik_potential_and_precision(lik, qΩ, y, f))
expected_auglik_precision(lik::AbstractLikelihood, qΩ, y::ROCArray, f=nothing) =
    last(expected_auglik_potential_and_precision(lik, qΩ, y, f))

# ------------------------------------------------------------------------------------------------ ELBO terms
# logtilt generic.jl:40-46 -> agpl_logtilt ; aug_loglik generic.jl:48-50 -> agpl_aug_loglik
function logtilt(lik::AbstractLikelihood, Ω::TupleVector, y::ROCArray, f::ROCArray{Float64})
    c = ctx()
    d, keep = desc(lik)
    out = Ref{Float64}(0.0)
    n = field(Ω, :n)
    GC.@preserve keep check(c.h, ccall((:agpl_logtilt, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}),
        c.h, d, npoints(lik, f), dptr(y), dptr(flat(Ω.ω)), dptr(n === nothing ? nothing : flat(n)), dptr(f), out))
    return out[]
end
function aug_loglik(lik::AbstractLikelihood, Ω::TupleVector, y::ROCArray, f::ROCArray{Float64})
    c = ctx()
    d, keep = desc(lik)
    out = Ref{Float64}(0.0)
    n = field(Ω, :n)
    GC.@preserve keep check(c.h, ccall((:agpl_aug_loglik, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}),
        c.h, d, npoints(lik, f), dptr(y), dptr(flat(Ω.ω)), dptr(n === nothing ? nothing : flat(n)), dptr(f), out))
    return out[]
end
# expected_logtilt api.jl:219-223 -> agpl_expected_logtilt
function expected_logtilt(lik::AbstractLikelihood, qΩ, y::ROCArray, qf::DeviceNormals)
    c = ctx()
    d, keep = desc(lik)
    φ = only(qΩ.inds)
    o2 = out2(φ)
    out = Ref{Float64}(0.0)
    GC.@preserve keep check(c.h, ccall((:agpl_expected_logtilt, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}),
        c.h, d, npoints(lik, qf.mean), dptr(y), dptr(flat(out1(lik, φ))), dptr(o2 === nothing ? nothing : flat(o2)),
        dptr(qf.mean), dptr(qf.var), out))
    return out[]
end
# aux_kldivergence(lik, qΩ, y) generic.jl:56-62 -> agpl_aux_kldivergence
function aux_kldivergence(lik::AbstractLikelihood, qΩ, y::ROCArray)
    c = ctx()
    d, keep = desc(lik)
    φ = only(qΩ.inds)
    o2 = out2(φ)
    out = Ref{Float64}(0.0)
    N = length(y) ÷ (lik isa CategoricalLikelihood ? nlatent(lik) : 1)
    GC.@preserve keep check(c.h, ccall((:agpl_aux_kldivergence, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}),
        c.h, d, N, dptr(y), dptr(flat(out1(lik, φ))), dptr(o2 === nothing ? nothing : flat(o2)), out))
    return out[]
end

# expected_aug_loglik(lik, qΩ, y, qf) generic.jl:52-54 (heteroscedasticgaussian.jl:130-145 its own method) -> agpl_expected_aug_loglik
function expected_aug_loglik(lik::AbstractLikelihood, qΩ, y::ROCArray, qf::DeviceNormals)
    c = ctx()
    d, keep = desc(lik)
    φ = only(qΩ.inds)
    o2 = out2(φ)
    out = Ref{Float64}(0.0)
    GC.@preserve keep check(c.h, ccall((:agpl_expected_aug_loglik, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}),
        c.h, d, npoints(lik, qf.mean), dptr(y), dptr(flat(out1(lik, φ))), dptr(o2 === nothing ? nothing : flat(o2)),
        dptr(qf.mean), dptr(qf.var), out))
    return out[]
end

# ------------------------------------------------------------------------------------------------ sparse sweep
"""
    SparseSweep(lik, Φ, d, y; comm=C_NULL, track_elbo=false)

State of the sparse CAVI loop (`cavi!`, examples/bernoulli/script.jl:29-39, in the sparse whitened form of
docs/src/index.md:154-163) on the shipped device path, i.e. ONE plan (include/agpl.h, agpl_plan_create): Φ::ROCMatrix{Float32}
is M x N column-major -- exactly Julia's layout of K_ZX (whitened: Φ = L⁻¹ K_ZX), any M (the plan zero-pads to a multiple of 256
inside; G, g stay M-sized) -- `d` the
Nyström residual k_nn - |φ_n|².  The plan builds both split-float16 images of Φ (one scale) and carries q(v) as (U, v) with
S = UᵀU, m = Uᵀv; after construction Φ itself is no longer read by the sweep and may be freed by the caller.
"""
mutable struct SparseSweep{Tlik}
    lik::Tlik
    plan::Ptr{Cvoid}            # agpl_plan*
    mem::ROCVector{UInt8}       # the plan's device memory (caller-owned storage: freed with this object)
    N::Int
    M::Int
    y::ROCArray
    Gg::ROCVector{Float64}      # [G (L M M) | g (L M) | ELBO terms (1)]: ONE buffer, one all-reduce per sweep
    kl::ROCVector{Float64}      # KL(q(v) || p(v)) of the last two updates
    nsweeps::Int
    track_elbo::Bool
    comm::Ptr{Cvoid}            # ncclComm_t when N is sharded over ranks, else C_NULL
end

function SparseSweep(lik, Φ::ROCMatrix{Float32}, d::ROCVector{Float32}, y::ROCArray; comm::Ptr{Cvoid}=C_NULL,
                     track_elbo::Bool=false)
    c = ctx()
    M, N = size(Φ)
    L = nlatent(lik)
    nbytes = ccall((:agpl_plan_bytes, libagpl), Int64, (Int64, Int32, Int32, UInt32), N, M, L, 0)
    nbytes > 0 || throw(ArgumentError("need N >= 1 points, M >= 1 features and nlatent <= 64 (got N = $N, M = $M)"))
    mem = ROCVector{UInt8}(undef, nbytes)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(c.h, ccall((:agpl_plan_create, libagpl), Int32,
        (Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, UInt32, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
        c.h, N, M, L, dptr(Φ), dptr(d), 0, dptr(mem), h))          # DomainError: a feature is not finite / out of range
    s = SparseSweep(lik, h[], mem, N, M, y, AMDGPU.zeros(Float64, L * M * M + L * M + 1), AMDGPU.zeros(Float64, 2), 0,
                    track_elbo, comm)
    finalizer(x -> ccall((:agpl_plan_destroy, libagpl), Int32, (Ptr{Cvoid},), x.plan), s)
    return s                                                       # q(v) = N(0, I) (script.jl:41-42)
end
Gview(s::SparseSweep) = (M = s.M; L = nlatent(s.lik); reshape(view(s.Gg, 1:(L * M * M)), M, M, L))
gview(s::SparseSweep) = (M = s.M; L = nlatent(s.lik); reshape(view(s.Gg, (L * M * M + 1):(L * M * M + L * M)), M, L))
Gptr(s::SparseSweep) = Ptr{Cvoid}(UInt(pointer(s.Gg)))
gptr(s::SparseSweep) = Ptr{Cvoid}(UInt(pointer(s.Gg)) + 8 * nlatent(s.lik) * s.M * s.M)
eptr(s::SparseSweep) = s.track_elbo ? Ptr{Cvoid}(UInt(pointer(s.Gg)) + 8 * (length(s.Gg) - 1)) : C_NULL

# S = (I + G)⁻¹, m = S g (script.jl:35-36) in factor form; enqueue only (a PosDefException surfaces in the next pass)
function update!(s::SparseSweep)
    c = ctx()
    kl = s.track_elbo ? Ptr{Cvoid}(UInt(pointer(s.kl)) + 8 * (s.nsweeps & 1)) : C_NULL
    return check(c.h, ccall((:agpl_plan_update, libagpl), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), s.plan, Gptr(s), gptr(s), C_NULL, kl))
end

# one sweep: marginals -> aux_posterior! -> expected potential / precision -> (G, g) -> [all-reduce] -> update
function sweep!(s::SparseSweep)
    c = ctx()
    L = nlatent(s.lik)
    dsc, keep = desc(s.lik)
    GC.@preserve keep check(c.h, ccall((:agpl_cavi_pass_plan, libagpl), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{Cvoid}),
        s.plan, dsc, C_NULL, dptr(s.y), Gptr(s), gptr(s), C_NULL, C_NULL, C_NULL, eptr(s)))
    if s.comm != C_NULL                           # the one exchange step of the N-sharded sweep (SURVEY.md 8e)
        check(c.h, ccall((:agpl_allreduce_nat, libagpl), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
                         c.h, s.comm, Gptr(s), length(s.Gg)))
    end
    update!(s)
    s.nsweeps += 1
    return s
end

function cavi!(s::SparseSweep; niter::Integer=10)
    for _ in 1:niter
        sweep!(s)
    end
    synchronize()                                 # the last update's outcome (PosDefException, ...)
    return moments(s)
end

"q(v) = N(m, S): m = Uᵀ v, S = Uᵀ U per latent, on the host (M x M)."
function moments(s::SparseSweep)
    synchronize()
    L, M = nlatent(s.lik), s.M
    U_p, v_p = Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Float64}}(C_NULL)
    check(ctx().h, ccall((:agpl_plan_state, libagpl), Int32,
                         (Ptr{Cvoid}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                         s.plan, U_p, v_p, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
    Mp = 256 * cld(M, 256)      # the plan's state arrays are sized by M rounded up to a multiple of 256 (include/agpl.h)
    A = Array(unsafe_wrap(ROCArray, U_p[], (Mp, Mp, L)))[1:M, 1:M, :]   # the caller's U: the leading M x M block
    v = Array(unsafe_wrap(ROCArray, v_p[], (Mp, L)))[1:M, :]
    U = [LowerTriangular(A[:, :, l]) for l in 1:L]
    return [U[l]' * v[:, l] for l in 1:L], [U[l]' * U[l] for l in 1:L]
end

"`marginals(post_u(x))` on the device (examples/bernoulli/script.jl:32-33): q(f_n) for the current (U, v)."
function device_marginals(s::SparseSweep)
    c = ctx()
    L = nlatent(s.lik)
    μ, σ² = ROCArray{Float32}(undef, s.N, L), ROCArray{Float32}(undef, s.N, L)
    check(c.h, ccall((:agpl_marginals_plan, libagpl), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        s.plan, C_NULL, dptr(μ), dptr(σ²)))
    # [N, L] latent-major out; the per-point operators take [L, N] (L contiguous per point)
    qm, qv = Float64.(permutedims(μ)), Float64.(permutedims(σ²))
    return L == 1 ? DeviceNormals(vec(qm), vec(qv)) : DeviceNormals(qm, qv)
end

"""
    device_loo_cavity(s::SparseSweep, γ, β) -> (μ, σ², h, Σh, n_bad, first_bad)

The leave-one-out cavity of the sweep's q(v) at its own points (agpl_plan_loo, include/agpl_loo.h): site i taken out of q(v) by a
rank-one downdate, from one marginal pass.  γ, β: Float32 [N, L] (latent-major), the sites of the q(v) the plan holds -- gamma_out /
beta_out of the pass whose G, g the last update was given.  μ, σ², h: Float64 [L, N] (L contiguous per point, what the per-point
operators and agpl_predictive take; NaN where a pair has no cavity); Σh: the leverage sums per latent on the host; n_bad and the
lowest (zero-based) flat index l N + i of a pair without a cavity (-1: none).
"""
function device_loo_cavity(s::SparseSweep, γ::ROCArray{Float32}, β::ROCArray{Float32})
    c = ctx()
    L = nlatent(s.lik)
    nbytes = ccall((:agpl_plan_loo_bytes, libagpl_loo), Int64, (Int64, Int32), s.N, L)
    nbytes > 0 || throw(ArgumentError("need N >= 1 points and 1 <= L <= 64 latents"))
    work = ROCVector{UInt8}(undef, nbytes)
    μ, σ², h = ROCArray{Float64}(undef, L, s.N), ROCArray{Float64}(undef, L, s.N), ROCArray{Float64}(undef, L, s.N)
    Σh = ROCVector{Float64}(undef, L)
    info = ROCVector{Int64}(undef, 2)
    check(c.h, ccall((:agpl_plan_loo, libagpl_loo), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        s.plan, C_NULL, dptr(γ), dptr(β), dptr(work), nbytes, dptr(μ), dptr(σ²), dptr(h), dptr(Σh), dptr(info)))
    bad = Array(info)
    return μ, σ², h, Array(Σh), Int(bad[1]), Int(bad[2])
end

"""
    SparseSweep(lik, x, z, ℓ, y; variance=1.0, jitter=1e-8)

The plan of the squared-exponential model straight from its raw inputs (agpl_plan_create_se): x [D, N], z [D, M] (Float64,
one column per point), ℓ D lengthscales; K_ZX and the whitened features never exist in device memory.  Such a sweep also
predicts (`device_predict`)."""
function SparseSweep(lik, x::ROCMatrix{Float64}, z::ROCMatrix{Float64}, ℓ::ROCVector{Float64}, y::ROCArray;
                     variance::Real=1.0, jitter::Real=1e-8, comm::Ptr{Cvoid}=C_NULL, track_elbo::Bool=false)
    c = ctx()
    D, N = size(x)
    M = size(z, 2)
    L = nlatent(lik)
    nbytes = ccall((:agpl_plan_se_bytes, libagpl_se), Int64, (Int64, Int32, Int32, Int32, UInt32), N, M, L, D, 0)
    nbytes > 0 || throw(ArgumentError("need N >= 1 points, M >= 1 inducing points, 1 <= D <= 16 and nlatent <= 64"))
    mem = ROCVector{UInt8}(undef, nbytes)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(c.h, ccall((:agpl_plan_create_se, libagpl_se), Int32,
        (Ptr{Cvoid}, Int64, Int32, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, UInt32, Ptr{Cvoid},
         Ref{Ptr{Cvoid}}),
        c.h, N, M, L, D, dptr(x), dptr(z), dptr(ℓ), variance, jitter, 0, dptr(mem), h))  # PosDefException, DomainError
    s = SparseSweep(lik, h[], mem, N, M, y, AMDGPU.zeros(Float64, L * M * M + L * M + 1), AMDGPU.zeros(Float64, 2), 0,
                    track_elbo, comm)
    finalizer(x -> ccall((:agpl_plan_destroy, libagpl), Int32, (Ptr{Cvoid},), x.plan), s)
    return s
end

# (kind, param) of include/agpl_kernels.h per base kernel of KernelFunctions.jl (Matern12Kernel is its alias of ExponentialKernel)
kernel_kind(::SqExponentialKernel) = (Int32(0), 0.0)
kernel_kind(::ExponentialKernel) = (Int32(1), 0.0)
kernel_kind(::Matern32Kernel) = (Int32(2), 0.0)
kernel_kind(::Matern52Kernel) = (Int32(3), 0.0)
kernel_kind(k::RationalQuadraticKernel) = (Int32(4), Float64(only(k.α)))
const AGPL_KERNEL_PERIODIC = Int32(6)  # include/agpl_kernels.h: PeriodicKernel(r = ℓ) on x / p, param = p (the constant only: no method maps to it yet; like the rest of this file, never executed here)
const AGPL_KERNEL_SE_COSINE = Int32(10)  # include/agpl_kernels.h: SqExponentialKernel ∘ ARDTransform times CosineKernel ∘ ScaleTransform(2 / p) on x[end], param = p (the constant only: no method maps to it yet)
const AGPL_KERNEL_SE_PERIODIC = Int32(8)  # include/agpl_kernels.h: SqExponentialKernel on x[1:end-1] ⊗ PeriodicKernel on x[end] / p, param = p (the constant only: no method maps to it yet)

"""
    SparseSweep(lik, kernel, x, z, ℓ, y; variance=1.0, jitter=1e-8)

The plan of `variance * with_lengthscale(kernel, ℓ)` straight from its raw inputs (agpl_plan_create_stationary) for `kernel` one of
`SqExponentialKernel()`, `ExponentialKernel()` / `Matern12Kernel()`, `Matern32Kernel()`, `Matern52Kernel()`,
`RationalQuadraticKernel(; α)`: the kernel of examples/bernoulli/script.jl:15 exchanged, everything else as the method above.
`device_predict` and `device_predict_chain` serve such a sweep with its kernel."""
function SparseSweep(lik, kernel, x::ROCMatrix{Float64}, z::ROCMatrix{Float64}, ℓ::ROCVector{Float64}, y::ROCArray;
                     variance::Real=1.0, jitter::Real=1e-8, comm::Ptr{Cvoid}=C_NULL, track_elbo::Bool=false)
    c = ctx()
    kind, param = kernel_kind(kernel)
    D, N = size(x)
    M = size(z, 2)
    L = nlatent(lik)
    nbytes = ccall((:agpl_plan_se_bytes, libagpl_se), Int64, (Int64, Int32, Int32, Int32, UInt32), N, M, L, D, 0)   # (every kind)
    nbytes > 0 || throw(ArgumentError("need N >= 1 points, M >= 1 inducing points, 1 <= D <= 16 and nlatent <= 64"))
    mem = ROCVector{UInt8}(undef, nbytes)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(c.h, ccall((:agpl_plan_create_stationary, libagpl_kernels), Int32,
        (Ptr{Cvoid}, Int64, Int32, Int32, Int32, Int32, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, UInt32,
         Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
        c.h, N, M, L, D, kind, param, dptr(x), dptr(z), dptr(ℓ), variance, jitter, 0, dptr(mem), h))
    s = SparseSweep(lik, h[], mem, N, M, y, AMDGPU.zeros(Float64, L * M * M + L * M + 1), AMDGPU.zeros(Float64, 2), 0,
                    track_elbo, comm)
    finalizer(x -> ccall((:agpl_plan_destroy, libagpl), Int32, (Ptr{Cvoid},), x.plan), s)
    return s
end

"`u_posterior(fz, m, S)(x_te)` marginals (examples/bernoulli/script.jl:46-56) at new inputs x_s [D, Ns] (agpl_plan_predict)."
function device_predict(s::SparseSweep, x_s::ROCMatrix{Float64})
    c = ctx()
    L, Ns = nlatent(s.lik), size(x_s, 2)
    μ, σ² = ROCArray{Float32}(undef, Ns, L), ROCArray{Float32}(undef, Ns, L)
    check(c.h, ccall((:agpl_plan_predict, libagpl_se), Int32, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        s.plan, Ns, dptr(x_s), C_NULL, dptr(μ), dptr(σ²)))
    qm, qv = Float64.(permutedims(μ)), Float64.(permutedims(σ²))
    return L == 1 ? DeviceNormals(vec(qm), vec(qv)) : DeviceNormals(qm, qv)
end

"""
    device_predict_chain(s, V, x_s; samples=false) -> (mean, var, resid[, F])

The posterior of f at new inputs x_s [D, Ns] from a chain of inducing draws V [M, L, T] (Float64; the Gibbs samples turned into a
posterior at x_te, examples/bernoulli/script.jl after `gibbs_sample`): the equal-weight mixture over t of N(φ' v_t, resid)
(agpl_plan_predict_chain).  `mean`, `var = resid + spread` are [Ns, L] Float32, `resid` [Ns]; `F` [Ns, L, T] the per-draw means.
"""
function device_predict_chain(s::SparseSweep, V::ROCArray{Float64}, x_s::ROCMatrix{Float64}; samples::Bool=false)
    c = ctx()
    L, Ns, T = nlatent(s.lik), size(x_s, 2), size(V, ndims(V))
    length(V) == s.M * L * T || throw(ArgumentError("the chain must be [M, L, T] = [$(s.M), $L, T]"))
    μ, spread = ROCArray{Float32}(undef, Ns, L), ROCArray{Float32}(undef, Ns, L)
    resid = ROCArray{Float32}(undef, Ns)
    F = samples ? ROCArray{Float32}(undef, Ns, L, T) : nothing
    check(c.h, ccall((:agpl_plan_predict_chain, libagpl_chain), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        s.plan, T, dptr(V), Ns, dptr(x_s), C_NULL, dptr(μ), dptr(spread), dptr(resid), dptr(F)))  # DomainError: non-finite draw
    σ² = spread .+ resid
    return samples ? (μ, σ², resid, F) : (μ, σ², resid)
end

"""
    device_predict_cov(s, x_a[, x_b]) -> C

`cov(u_posterior(fz, m, S)(x_a), u_posterior(fz, m, S)(x_b))` (examples/bernoulli/script.jl:46-56) under the sweep's q(v), at inputs
x_a [D, Na] and x_b [D, Nb] (agpl_plan_predict_cov): C [Nb, Na, L] Float32, C[j, i, l] = Cov_l(f(x_a_i), f(x_b_j)) (the library's
row-major [L][Na][Nb]).  Without x_b: the symmetric form at x_b = x_a, symmetric bit for bit, whose diagonal is `device_predict`'s
variance; `cholesky(Symmetric(Float64.(C[:, :, l]) + jitter * I)).L * randn(Na)` added to the mean is a coherent draw of f.
"""
function device_predict_cov(s::SparseSweep, x_a::ROCMatrix{Float64}, x_b::Union{ROCMatrix{Float64},Nothing}=nothing)
    c = ctx()
    L, Na = nlatent(s.lik), size(x_a, 2)
    Nb = x_b === nothing ? Na : size(x_b, 2)
    C = ROCArray{Float32}(undef, Nb, Na, L)
    check(c.h, ccall((:agpl_plan_predict_cov, libagpl_joint), Int32,
        (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
        s.plan, Na, dptr(x_a), Nb, x_b === nothing ? C_NULL : dptr(x_b), dptr(C), Nb))
    return C
end

"""
    device_predict_grad(s, x_s) -> (dμ, dσ²)

The posterior of the gradient of f under the sweep's q(v) at new inputs x_s [D, Ns] (agpl_plan_predict_grad, include/agpl_grad.h):
dμ[i, d, l] = E ∂f_l/∂x_d (x_i) and dσ²[i, d, l] = Var ∂f_l/∂x_d (x_i), [Ns, D, L] Float32 each (the library's row-major [L][D][Ns]) --
a closed-form Gaussian, not a difference quotient of `device_predict`.  Any kernel of the plan but Matern-1/2 (not differentiable:
the call throws).  The gradient of a prior mean function is the caller's to add to dμ.
"""
function device_predict_grad(s::SparseSweep, x_s::ROCMatrix{Float64})
    c = ctx()
    L, (D, Ns) = nlatent(s.lik), size(x_s)
    dμ, dσ² = ROCArray{Float32}(undef, Ns, D, L), ROCArray{Float32}(undef, Ns, D, L)
    check(c.h, ccall((:agpl_plan_predict_grad, libagpl_grad), Int32, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        s.plan, Ns, dptr(x_s), dptr(dμ), dptr(dσ²)))
    return dμ, dσ²
end

"""
    device_select_inducing(x, M, lengthscale; niter=10, z0=nothing) -> z

Inducing inputs from the data (agpl_select_inducing_kmeans, include/agpl_inducing.h): M centres of Lloyd's k-means over the columns
of x [D, N] in the metric x ./ lengthscale, from a stratified start of the context's seed (or `z0` [D, M]); z [D, M] on the device,
the same bits however the points would be split over ranks.  `lengthscale` is a host vector of D numbers.
"""
function device_select_inducing(x::ROCMatrix{Float64}, M::Integer, lengthscale::Vector{Float64}; niter::Integer=10,
                                z0::Union{ROCMatrix{Float64},Nothing}=nothing)
    c = ctx()
    D, N = size(x)
    length(lengthscale) == D || throw(ArgumentError("lengthscale must have D = $D entries"))
    z = ROCArray{Float64}(undef, D, M)
    GC.@preserve lengthscale check(c.h, ccall((:agpl_select_inducing_kmeans, libagpl_inducing), Int32,
        (Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, N, M, D, dptr(x), Ptr{Cvoid}(pointer(lengthscale)), niter, z0 === nothing ? C_NULL : dptr(z0), dptr(z), C_NULL))
    return z
end

"""
    device_select_inducing_greedy(x, M, kernel, lengthscale; variance=1.0, threshold=1e-6) -> (z, indices, info)

Inducing inputs from the data by greedy conditional variance, the partial pivoted Cholesky of K_XX (agpl_select_inducing_greedy,
include/agpl_greedy.h): repeatedly the column of x [D, N] whose prior variance given the inputs chosen so far is largest, until M are
chosen or that variance is at most `threshold * variance`.  z [D, m] on the device, their (zero-based) indices, and the header's
info vector [1 + 2M] on the host (m; max d / variance before each pick; tr(K - Q) / variance after each pick).  `kernel` as for the
plans from raw inputs; `lengthscale` is a host vector of D numbers.
"""
function device_select_inducing_greedy(x::ROCMatrix{Float64}, M::Integer, kernel, lengthscale::Vector{Float64};
                                       variance::Real=1.0, threshold::Real=1e-6)
    c = ctx()
    D, N = size(x)
    length(lengthscale) == D || throw(ArgumentError("lengthscale must have D = $D entries"))
    kind, param = kernel_kind(kernel)
    nbytes = Ref{Int64}(0)
    ccall((:agpl_greedy_bytes, libagpl_greedy), Int32, (Int64, Int32, Ptr{Cvoid}), N, M, nbytes) == 0 ||
        throw(ArgumentError("need N >= 1 points and 1 <= M <= 2048"))
    work = ROCVector{UInt8}(undef, nbytes[])
    z = ROCArray{Float64}(undef, D, M)
    idx = ROCVector{Int64}(undef, M)
    info = ROCVector{Float64}(undef, 1 + 2M)
    GC.@preserve lengthscale check(c.h, ccall((:agpl_select_inducing_greedy, libagpl_greedy), Int32,
        (Ptr{Cvoid}, Int64, Int32, Int32, Int32, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, N, M, D, kind, param, dptr(x), Ptr{Cvoid}(pointer(lengthscale)), variance, threshold, dptr(work), nbytes[], dptr(z), dptr(idx), dptr(info)))
    h = Array(info)
    m = Int(h[1])
    return z[:, 1:m], Array(idx)[1:m], h
end

"""
    device_predictive(lik, qf::DeviceNormals, y=nothing; nsamples=0, sweep=0) -> (mean, var, logp, total)

The predictive distribution of y under q(f) (agpl_predictive): E[y], Var[y] and, with observations `y`, log p(yᵢ) per point and
their device sum.  Categorical likelihoods: `mean` holds the class probabilities [K, N], `var` is `nothing`.
"""
function device_predictive(lik::AbstractLikelihood, qf::DeviceNormals, y::Union{ROCArray,Nothing}=nothing; nsamples::Integer=0,
                           sweep::Integer=0)
    c = ctx()
    d, keep = desc(lik)
    n = npoints(lik, qf.mean)
    cat = d.kind == 3 || d.kind == 4
    μy = cat ? ROCArray{Float64}(undef, nlatent(lik) + (d.kind == 4 ? 1 : 0), n) : ROCArray{Float64}(undef, n)
    σ²y = cat ? nothing : ROCArray{Float64}(undef, n)
    logp = y === nothing ? nothing : ROCArray{Float64}(undef, n)
    total = y === nothing ? nothing : ROCArray{Float64}(undef, 1)
    GC.@preserve keep check(c.h, ccall((:agpl_predictive, libagpl_predictive), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, d, n, dptr(qf.mean), dptr(qf.var), dptr(y), nsamples, sweep, dptr(μy), dptr(σ²y), dptr(logp), dptr(total)))
    return μy, σ²y, logp, total === nothing ? nothing : Array(total)[1]
end

"""
    device_predictive_cdf(lik, qf::DeviceNormals, y) -> (cdf, sf)

P(Y ≤ yᵢ) and P(Y > yᵢ) of the predictive of y under q(f) (agpl_predictive_cdf, include/agpl_quantile.h), [N] Float64 each; the upper
tail is computed as such, not as 1 - cdf.  Every likelihood but the categorical ones, which are refused (ArgumentError): classes
have no order.  For a count y, cdf(y) - cdf(y - 1) is the probability of y.
"""
function device_predictive_cdf(lik::AbstractLikelihood, qf::DeviceNormals, y::ROCArray)
    c = ctx()
    d, keep = desc(lik)
    n = npoints(lik, qf.mean)
    cdf, sf = ROCArray{Float64}(undef, n), ROCArray{Float64}(undef, n)
    GC.@preserve keep check(c.h, ccall((:agpl_predictive_cdf, libagpl_quantile), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, d, n, dptr(qf.mean), dptr(qf.var), dptr(y), dptr(cdf), dptr(sf)))
    return cdf, sf
end

"""
    device_predictive_quantile(lik, qf::DeviceNormals, probs) -> q

Quantiles of the predictive of y under q(f) (agpl_predictive_quantile, include/agpl_quantile.h): q[j, i] = inf {y : P(Y ≤ y) ≥ probs[j]},
[nq, N] Float64 (the library's row-major [N][nq]); `probs` is a host vector of 1 to 16 numbers in (0, 1).
"""
function device_predictive_quantile(lik::AbstractLikelihood, qf::DeviceNormals, probs::Vector{Float64})
    c = ctx()
    d, keep = desc(lik)
    n, nq = npoints(lik, qf.mean), length(probs)
    p, q = ROCArray(probs), ROCArray{Float64}(undef, nq, n)
    GC.@preserve keep check(c.h, ccall((:agpl_predictive_quantile, libagpl_quantile), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, d, n, dptr(qf.mean), dptr(qf.var), nq, dptr(p), dptr(q)))
    return q
end

"""
    device_expected_loglik(lik, qf::DeviceNormals, y; per_point=false) -> (ell, grad[, ell_i, dell_i])

Σᵢ E_{q(fᵢ)} log p(yᵢ | fᵢ) and its gradient for the logarithms of the likelihood's parameters (agpl_expected_loglik), in the order of
the descriptor's `p`: Student-t (log ν, log σ), NegBinomial log r, Poisson / heteroscedastic log λ, Laplace log β; Bernoulli has
none (`grad` is empty).  The categorical likelihoods are refused (ArgumentError).  `per_point` adds the device arrays [N] and [P, N].
"""
function device_expected_loglik(lik::AbstractLikelihood, qf::DeviceNormals, y::ROCArray; per_point::Bool=false)
    c = ctx()
    d, keep = desc(lik)
    n = npoints(lik, qf.mean)
    P = d.kind == 0 ? 0 : (d.kind == 2 ? 2 : 1)
    ell = per_point ? ROCArray{Float64}(undef, n) : nothing
    dell = per_point && P > 0 ? ROCArray{Float64}(undef, P, n) : nothing
    total = ROCArray{Float64}(undef, 1)
    grad = P > 0 ? ROCArray{Float64}(undef, P) : nothing
    GC.@preserve keep check(c.h, ccall((:agpl_expected_loglik, libagpl_likgrad), Int32,
        (Ptr{Cvoid}, Ref{LikDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        c.h, d, n, dptr(qf.mean), dptr(qf.var), dptr(y), dptr(ell), dptr(dell), dptr(total), dptr(grad)))
    out = (Array(total)[1], grad === nothing ? Float64[] : Array(grad))
    return per_point ? (out..., ell, dell) : out
end

"The features the plan holds for points i0 + 1 .. i0 + n: Float32 [M, n] (agpl_plan_features)."
function device_features(s::SparseSweep, i0::Integer=0, n::Integer=s.N - i0)
    Φ = ROCArray{Float32}(undef, s.M, n)
    check(ctx().h, ccall((:agpl_plan_features, libagpl_se), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}), s.plan, i0, n, dptr(Φ)))
    return Φ
end

"""
`aug_elbo` (examples/bernoulli/script.jl:65-70) of the q(v) that ENTERED the last sweep, at no extra pass over Φ
(`track_elbo=true`): the per-point terms rode that sweep's per-point kernel (and its all-reduce), KL(q(v) ‖ p(v)) the update
that made that q(v).
"""
function elbo_entering(s::SparseSweep)
    (s.track_elbo && s.nsweeps > 0) || throw(ArgumentError("elbo_entering needs track_elbo=true and one sweep"))
    synchronize()
    return Array(view(s.Gg, length(s.Gg):length(s.Gg)))[1] - Array(s.kl)[(s.nsweeps & 1) + 1]
end

"`aug_elbo` of examples/bernoulli/script.jl:65-70 for the current q(v), by separate passes (the reference's own operators)."
function aug_elbo(s::SparseSweep)
    c = ctx()
    M = s.M
    L = nlatent(s.lik)
    qf = device_marginals(s)
    qΩ = AugmentedGPLikelihoods.init_aux_posterior(s.lik, s.N)
    qΩdev = to_device(qΩ)
    aux_posterior!(qΩdev, s.lik, s.y, qf)
    # KL(q(v) ‖ N(0, I)) = (tr S + mᵀm − M + log det(I + G)) / 2 from the plan's factor: S = UᵀU, m = Uᵀv, log det(S) = 2 Σ log U_aa
    ms, Ss = moments(s)
    kl = sum(0.5 * (tr(Ss[l]) + dot(ms[l], ms[l]) - M - logdet(Symmetric(Ss[l]))) for l in 1:L)
    return expected_logtilt(s.lik, qΩdev, s.y, qf) - aux_kldivergence(s.lik, qΩdev, s.y) - kl
end

"A `For(TupleVector(...))` of host vectors -> the same container over device arrays (fields keep their names)."
function to_device(qΩ)
    φ = only(qΩ.inds)
    names = propertynames(φ)
    return (; inds=(TupleVectorLike(NamedTuple{names}(map(n -> ROCArray(flat(getproperty(φ, n))), names))),))
end
struct TupleVectorLike{NT<:NamedTuple}
    fields::NT
end
Base.getproperty(t::TupleVectorLike, s::Symbol) = s === :fields ? getfield(t, :fields) : getfield(t, :fields)[s]
Base.hasproperty(t::TupleVectorLike, s::Symbol) = haskey(getfield(t, :fields), s)
Base.propertynames(t::TupleVectorLike) = keys(getfield(t, :fields))

end # module
