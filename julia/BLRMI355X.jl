# BLRMI355X.jl -- the Julia side of the drop-in boundary (NOT runnable in the build image: no `julia`).
#
# Kept deliberately thin so it is correct by inspection: every behaviour it relies on is exercised through the same C ABI
# by the Python/ctypes harness (tests/test_gpu_parity.py), and tests/test_abi_cpu.py keeps every ccall below in step with
# include/blr_mi355x.h (argument count and kind per position).
#
# What it offloads, for FiniteGP{<:BayesianLinearRegressor} / FiniteGP{<:BasisFunctionRegressor} with Float64 / Float32 data,
# ColVecs / RowVecs inputs, Diagonal (incl. Fill) or dense observation noise:
#     logpdf(fx, y), logpdf(fx, Y::Matrix), posterior(fx, y), mean, var, cov, mean_and_var, mean_and_cov, marginals,
#     rand(rng, fx[, S]), rand(rng, f[, dims]), rand!(rng, A, f), Random.Sampler          (reference src/*.jl, cited per function)
# plus what the reference gets from Zygote and a ccall cannot give by itself:
#     ChainRulesCore.rrule(logpdf, fx, y)                                                     (README.md:56-71, examples/nn-blr.jl:35-37)
# and what only a device library can offer:
#     maps over collections of problems in one call (logpdf_map, posterior_map), device-resident batches (posterior_batched!), the RCCL exchange for one Julia process per GPU (comm_init!, logpdf_allgather_sum!).
# Anything else (exotic element types, unknown containers) falls back to the reference's own CPU methods.
#
# Two ways to use it -- both spelled out in INTEGRATION.md:
#   opt-in, side by side :  using .BLRMI355X;  BLRMI355X.logpdf(fx, y)
#   drop-in              :  BLRMI355X.install_overrides!()  replaces the reference's methods on FiniteGP{<:BayesianLinearRegressor}
#                           (src/bayesian_linear_regression.jl:33-69) by the offloaded ones for the whole session.
module BLRMI355X

using AbstractGPs, LinearAlgebra, PDMats, Random
using AbstractGPs: FiniteGP
using BayesianLinearRegressors: BayesianLinearRegressor, BasisFunctionRegressor, BLRFunctionSample
import BayesianLinearRegressors as REF
import ChainRulesCore
using ChainRulesCore: NoTangent, Tangent, ZeroTangent

const LIB = get(ENV, "BLR_MI355X_LIB", "libblr_mi355x")

# enums of include/blr_mi355x.h
const COLVECS, ROWVECS = Cint(0), Cint(1)
const ISOTROPIC, DIAGONALN, DENSEN = Cint(0), Cint(1), Cint(2)
const P_DENSE, P_UPPER, P_DIAG = Cint(0), Cint(1), Cint(2)
const MEM_HOST, MEM_DEVICE = Cint(0), Cint(1)

const Elt = Union{Float32,Float64}
const FiniteBLR = FiniteGP{<:Union{BayesianLinearRegressor,BasisFunctionRegressor}}

# ---- handle: one per task ------------------------------------------------------------------------------
const HANDLE_KEY = :blr_mi355x_handle
function handle()
    get!(task_local_storage(), HANDLE_KEY) do
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:blr_create, LIB), Cint, (Cint, Ref{Ptr{Cvoid}}), parse(Cint, get(ENV, "BLR_MI355X_DEVICE", "0")), h)
        rc == 0 || error("blr_create failed with code $rc (no MI355X visible?)")
        h[]
    end::Ptr{Cvoid}
end

function check(h, rc)
    rc == 0 && return nothing
    rc > 0 && throw(PosDefException(rc))                       # what cholesky at reference :78/:79/:86 throws
    msg = unsafe_string(ccall((:blr_last_error, LIB), Cstring, (Ptr{Cvoid},), h))
    rc > -1000 ? throw(DimensionMismatch("libblr_mi355x: $msg")) : error("libblr_mi355x (HIP/RCCL): $msg")
end

# ---- x_as_colvecs (reference :20-31) as (array, layout, ld, D, N): zero copies -----------------------------
xlayout(x::ColVecs{T,<:StridedMatrix{T}}) where {T<:Elt} = (x.X, COLVECS, stride(x.X, 2), size(x.X, 1), size(x.X, 2))
xlayout(x::RowVecs{T,<:StridedMatrix{T}}) where {T<:Elt} = (x.X, ROWVECS, stride(x.X, 2), size(x.X, 2), size(x.X, 1))
xlayout(x) = nothing  # anything else: not offloadable (the reference raises its own error for unknown containers)

# observation noise -> (buffer, kind, leading dimension)
noise(Σ::Diagonal{T,<:AbstractGPs.FillArrays.Fill}) where {T<:Elt} = (T[Σ.diag.value], ISOTROPIC, 1)
noise(Σ::Diagonal{T,<:StridedVector{T}}) where {T<:Elt} = (Σ.diag, DIAGONALN, 1)
noise(Σ::StridedMatrix{T}) where {T<:Elt} = (Σ, DENSEN, stride(Σ, 2))                  # reference :79-82 general branch
noise(Σ::Symmetric{T,<:StridedMatrix{T}}) where {T<:Elt} = (Matrix(Σ), DENSEN, size(Σ, 1))
noise(Σ) = nothing

prior(Λ::Diagonal{T}) where {T<:Elt} = (collect(Λ.diag), P_DIAG, 1)
prior(Λ::PDMat{T}) where {T<:Elt} = (Matrix(Λ.chol.U), P_UPPER, size(Λ, 1))          # factor carried forward (:93)
prior(Λ::Symmetric{T,<:StridedMatrix{T}}) where {T<:Elt} = (Matrix(Λ), P_DENSE, size(Λ, 1))
prior(Λ::StridedMatrix{T}) where {T<:Elt} = (Λ, P_DENSE, stride(Λ, 2))
prior(Λ) = nothing

build_Λ(::Type{<:AbstractPDMat}, T, A) = PDMat(Cholesky(UpperTriangular(T)))           # reference :93
build_Λ(_, T, A) = Symmetric(A)                                                          # reference :92 (A == T'T)

to_blr(fx::FiniteGP{<:BayesianLinearRegressor}) = fx
to_blr(fx::FiniteGP{<:BasisFunctionRegressor}) = fx.f.blr(fx.f.ϕ(fx.x), fx.Σy)         # basis_function_regression.jl:41

# ---- random-Fourier basis on the device (BASELINE config 5) -----------------------------------------
# A BasisFunctionRegressor whose ϕ is  x -> sqrt(2/D) cos.(Ω'x .+ β)  (reference basis_function_regression.jl:41,62-65:
# bfr(x) = blr(ϕ(x))) hands the raw inputs to the device: the feature matrix is generated there and consumed by the same
# fused posterior/logpdf path, never crossing PCIe.
struct RandomFourierFeatures{T<:Elt}
    Ω::Matrix{T}      # Din x D
    β::Vector{T}      # D
end
(r::RandomFourierFeatures{T})(x::ColVecs) where {T} = ColVecs(convert(T, sqrt(2 / length(r.β))) .* cos.(r.Ω' * x.X .+ r.β))
(r::RandomFourierFeatures)(x::RowVecs) = r(ColVecs(permutedims(x.X)))

function fused_rff(blr::BayesianLinearRegressor, ϕ::RandomFourierFeatures{T}, x::ColVecs, Σy, y::AbstractVector, want_posterior::Bool) where {T}
    pr = prior(blr.Λw); nz = noise(Σy)
    (pr === nothing || nz === nothing || nz[2] == DENSEN) && return nothing
    Lw, pk, ldl = pr; s, nk, _ = nz
    Din, D = size(ϕ.Ω); N = length(y)
    Xin = convert(Matrix{T}, x.X); yv = convert(Vector{T}, y); mw = convert(Vector{T}, blr.mw)
    mw′ = want_posterior ? Vector{T}(undef, D) : Ptr{T}(C_NULL)
    Tm = want_posterior ? Matrix{T}(undef, D, D) : Ptr{T}(C_NULL)
    A = (want_posterior && pk != P_UPPER) ? Matrix{T}(undef, D, D) : Ptr{T}(C_NULL)
    lp = Ref{Cdouble}(0.0); info = Ref{Int32}(0)
    h = handle()
    rc = GC.@preserve Xin yv s Lw mw mw′ Tm A begin
        if T === Float64
            ccall((:blr_posterior_rff_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, T, Ptr{T}, Cint, Ptr{T},
                   Cint, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ref{Cdouble}, Ref{Int32}),
                  h, MEM_HOST, Din, D, N, Xin, Din, ϕ.Ω, Din, ϕ.β, sqrt(T(2) / D), yv, nk, s, pk, mw, Lw, ldl, mw′, Tm, D, A, D,
                  lp, info)
        else
            ccall((:blr_posterior_rff_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, T, Ptr{T}, Cint, Ptr{T},
                   Cint, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ref{Cdouble}, Ref{Int32}),
                  h, MEM_HOST, Din, D, N, Xin, Din, ϕ.Ω, Din, ϕ.β, sqrt(T(2) / D), yv, nk, s, pk, mw, Lw, ldl, mw′, Tm, D, A, D,
                  lp, info)
        end
    end
    check(h, rc)
    info[] > 0 && throw(PosDefException(info[]))
    return lp[], mw′, Tm, A
end

# ---- fused inference: reference :55-58, :60-69, :72-89 ------------------------------------------------------
function fused(fx::FiniteGP, y::AbstractVector{<:Real}, want_posterior::Bool)
    # BasisFunctionRegressor with the random-Fourier ϕ: features + inference in one library call
    if fx.f isa BasisFunctionRegressor && fx.f.ϕ isa RandomFourierFeatures && fx.x isa ColVecs
        r = fused_rff(fx.f.blr, fx.f.ϕ, fx.x, fx.Σy, y, want_posterior)
        r === nothing || return r
    end
    fb = to_blr(fx)
    xl, nz, pr = xlayout(fb.x), noise(fb.Σy), prior(fb.f.Λw)
    (xl === nothing || nz === nothing || pr === nothing) && return nothing
    X, layout, ldx, D, N = xl
    T = eltype(X)
    length(y) == N || throw(error("length(y) != size(fx.x.X, 2)"))                        # reference :74
    length(fb.f.mw) == D || throw(DimensionMismatch("length(mw) != dimension of the inputs"))
    yv, mw = convert(Vector{T}, y), convert(Vector{T}, fb.f.mw)
    s, nk, lds = nz
    Lw, pk, ldl = pr
    mw_post = want_posterior ? Vector{T}(undef, D) : Ptr{T}(C_NULL)
    Tp = want_posterior ? Matrix{T}(undef, D, D) : Ptr{T}(C_NULL)
    Ap = (want_posterior && pk != P_UPPER) ? Matrix{T}(undef, D, D) : Ptr{T}(C_NULL)
    lp = Ref{Cdouble}(0.0)
    h = handle()
    if nk == DENSEN                                                                        # reference :79-82, general Sigma_y
        info = Ref{Int32}(0)
        rc = GC.@preserve X yv mw s Lw mw_post Tp Ap begin
            if T === Float64
                ccall((:blr_posterior_dense_noise_f64, LIB), Cint,
                      (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Ptr{T}, Int64, Cint, Ptr{T}, Ptr{T}, Int64,
                       Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ref{Cdouble}, Ref{Int32}),
                      h, MEM_HOST, layout, D, N, X, ldx, yv, s, lds, pk, mw, Lw, ldl, mw_post, Tp, D, Ap, D, lp, info)
            else
                ccall((:blr_posterior_dense_noise_f32, LIB), Cint,
                      (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Ptr{T}, Int64, Cint, Ptr{T}, Ptr{T}, Int64,
                       Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ref{Cdouble}, Ref{Int32}),
                      h, MEM_HOST, layout, D, N, X, ldx, yv, s, lds, pk, mw, Lw, ldl, mw_post, Tp, D, Ap, D, lp, info)
            end
        end
        check(h, rc)
        check(h, info[])
        return lp[], mw_post, Tp, Ap
    end
    rc = GC.@preserve X yv mw s Lw mw_post Tp Ap begin
        if T === Float64
            ccall((:blr_posterior_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Cint, Ptr{T}, Ptr{T}, Int64,
                   Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ref{Cdouble}),
                  h, layout, D, N, X, ldx, yv, nk, s, pk, mw, Lw, ldl, mw_post, Tp, D, Ap, D, lp)
        else
            ccall((:blr_posterior_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Cint, Ptr{T}, Ptr{T}, Int64,
                   Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ref{Cdouble}),
                  h, layout, D, N, X, ldx, yv, nk, s, pk, mw, Lw, ldl, mw_post, Tp, D, Ap, D, lp)
        end
    end
    check(h, rc)
    return lp[], mw_post, Tp, Ap
end

function logpdf(fx::FiniteGP, y::AbstractVector{<:Real})
    r = fused(fx, y, false)
    r === nothing ? REF_logpdf(fx, y) : r[1]
end

function posterior(fx::FiniteGP, y::AbstractVector{<:Real})
    r = fused(fx, y, true)
    r === nothing && return REF_posterior(fx, y)
    _, mw_post, Tp, Ap = r
    blr0 = fx.f isa BasisFunctionRegressor ? fx.f.blr : fx.f
    post = BayesianLinearRegressor(mw_post, build_Λ(typeof(blr0.Λw), Tp, Ap))
    fx.f isa BasisFunctionRegressor ? BasisFunctionRegressor(post, fx.f.ϕ) : post           # :62-65
end

# ---- many problems in ONE library call: `map(posterior, fxs, ys)` / `logpdf.(fxs, ys)` -------------------
# (BASELINE config 4 is this with 8192 regressors; at D > 128 the regressors share every launch of the update.)  Host arrays
# are packed side by side -- problem b at b * stride -- and handed to blr_posterior_batched_* with BLR_MEM_HOST; problems that
# differ only in their number of observations go to blr_posterior_ragged_* (fused_ragged).  Collections neither entry point
# takes (mixed layouts / kinds, dense noise, a fused random-Fourier basis) are mapped one by one.  The first problem that is not positive definite throws PosDefException, as the map would.
function fused_many(fxs::AbstractVector{<:FiniteGP}, ys::AbstractVector{<:AbstractVector{<:Real}}, want_posterior::Bool)
    length(fxs) == length(ys) || throw(DimensionMismatch("as many observation vectors as finite regressors are needed"))
    B = length(fxs)
    B == 0 && return Tuple[]
    any(fx -> fx.f isa BasisFunctionRegressor && fx.f.ϕ isa RandomFourierFeatures, fxs) && return nothing
    fbs = map(to_blr, fxs)
    xls, nzs, prs = map(fb -> xlayout(fb.x), fbs), map(fb -> noise(fb.Σy), fbs), map(fb -> prior(fb.f.Λw), fbs)
    (any(isnothing, xls) || any(isnothing, nzs) || any(isnothing, prs)) && return nothing
    X1, layout, _, D, N = xls[1]
    T = eltype(X1)
    nk, pk = nzs[1][2], prs[1][2]
    (nk == DENSEN || D == 0) && return nothing
    alike = all(b -> eltype(xls[b][1]) === T && xls[b][2] == layout && xls[b][4] == D && nzs[b][2] == nk &&
                     prs[b][2] == pk && length(ys[b]) == xls[b][5] && length(fbs[b].f.mw) == D, 1:B)
    alike || return nothing
    # everything but the number of observations agrees: ONE blr_posterior_ragged_* call on the packed observations
    all(b -> xls[b][5] == N, 1:B) || return fused_ragged(fbs, ys, xls, nzs, prs, want_posterior)
    N == 0 && return nothing
    rows, cols = layout == COLVECS ? (D, N) : (N, D)
    Xb = Array{T}(undef, rows, cols, B)
    for b in 1:B
        copyto!(view(Xb, :, :, b), xls[b][1])
    end
    yb = Matrix{T}(undef, N, B)
    for b in 1:B
        yb[:, b] .= ys[b]
    end
    ns = nk == ISOTROPIC ? 1 : N
    sb = Matrix{T}(undef, ns, B)
    for b in 1:B
        sb[:, b] .= view(nzs[b][1], 1:ns)
    end
    mwb = Matrix{T}(undef, D, B)
    for b in 1:B
        mwb[:, b] .= fbs[b].f.mw
    end
    Lb = pk == P_DIAG ? Matrix{T}(undef, D, B) : Array{T}(undef, D, D, B)
    for b in 1:B
        pk == P_DIAG ? (Lb[:, b] .= prs[b][1]) : copyto!(view(Lb, :, :, b), prs[b][1])
    end
    ldl, strideL = pk == P_DIAG ? (1, D) : (D, D * D)
    mw_post = want_posterior ? Matrix{T}(undef, D, B) : Ptr{T}(C_NULL)
    Tp = want_posterior ? Array{T}(undef, D, D, B) : Ptr{T}(C_NULL)
    Ap = (want_posterior && pk != P_UPPER) ? Array{T}(undef, D, D, B) : Ptr{T}(C_NULL)
    lp = zeros(Cdouble, B)
    info = zeros(Int32, B)
    h = handle()
    rc = GC.@preserve Xb yb sb mwb Lb mw_post Tp Ap lp info begin
        if T === Float64
            ccall((:blr_posterior_batched_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
                  h, MEM_HOST, layout, B, D, N, Xb, rows, rows * cols, yb, N, nk, sb, ns, pk, mwb, D, Lb, ldl, strideL,
                  mw_post, D, Tp, D, D * D, Ap, D, D * D, lp, info)
        else
            ccall((:blr_posterior_batched_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
                  h, MEM_HOST, layout, B, D, N, Xb, rows, rows * cols, yb, N, nk, sb, ns, pk, mwb, D, Lb, ldl, strideL,
                  mw_post, D, Tp, D, D * D, Ap, D, D * D, lp, info)
        end
    end
    check(h, rc)
    bad = findfirst(>(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))
    want_posterior || return [(lp[b], nothing, nothing, nothing) for b in 1:B]
    return [(lp[b], mw_post[:, b], Tp[:, :, b], Ap isa Ptr ? Ap : Ap[:, :, b]) for b in 1:B]
end

# blr_posterior_ragged_* (include/blr_mi355x.h): B regressors with unequal observation counts, packed side by side; `offsets`
# (B + 1 entries, zero based) is ALWAYS a host array.  The other arrays are host Arrays (MEM_HOST) or raw device pointers.
function posterior_ragged_call(h, ::Type{T}, memspace, layout, B, D, offsets::Vector{Int64}, X, ldx, y, nk, s, strides, pk, mw, stridemw,
                               Lw, ldl, strideLw, mw_post, stride_mwpost, Tp, ldt, strideT, Ap, ldlp, strideLp, lp, info) where {T<:Elt}
    GC.@preserve offsets X y s mw Lw mw_post Tp Ap lp info begin
        if T === Float64
            ccall((:blr_posterior_ragged_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, y, nk, s, strides, pk, mw, stridemw,
                  Lw, ldl, strideLw, mw_post, stride_mwpost, Tp, ldt, strideT, Ap, ldlp, strideLp, lp, info)
        else
            ccall((:blr_posterior_ragged_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, y, nk, s, strides, pk, mw, stridemw,
                  Lw, ldl, strideLw, mw_post, stride_mwpost, Tp, ldt, strideT, Ap, ldlp, strideLp, lp, info)
        end
    end
end

# fused_many for problems that differ only in their number of observations (xls / nzs / prs: their xlayout / noise / prior)
function fused_ragged(fbs, ys, xls, nzs, prs, want_posterior::Bool)
    B = length(fbs)
    X1, layout, _, D, _ = xls[1]
    T = eltype(X1)
    nk, pk = nzs[1][2], prs[1][2]
    offsets = Int64[0; cumsum(Int64[xl[5] for xl in xls])]
    total = Int(offsets[end])
    # ColVecs: D x N_b blocks side by side; RowVecs: N_b x D blocks stacked by rows (one total x D column-major matrix)
    Xp = layout == COLVECS ? Matrix{T}(undef, D, total) : Matrix{T}(undef, total, D)
    yp = Vector{T}(undef, total)
    sp = Vector{T}(undef, nk == ISOTROPIC ? B : total)
    for b in 1:B
        r = (offsets[b] + 1):offsets[b + 1]
        copyto!(layout == COLVECS ? view(Xp, :, r) : view(Xp, r, :), xls[b][1])
        yp[r] .= ys[b]
        nk == ISOTROPIC ? (sp[b] = nzs[b][1][1]) : (sp[r] .= view(nzs[b][1], 1:length(r)))
    end
    mwb = Matrix{T}(undef, D, B)
    for b in 1:B
        mwb[:, b] .= fbs[b].f.mw
    end
    Lb = pk == P_DIAG ? Matrix{T}(undef, D, B) : Array{T}(undef, D, D, B)
    for b in 1:B
        pk == P_DIAG ? (Lb[:, b] .= prs[b][1]) : copyto!(view(Lb, :, :, b), prs[b][1])
    end
    ldl, strideL = pk == P_DIAG ? (1, D) : (D, D * D)
    mw_post = want_posterior ? Matrix{T}(undef, D, B) : Ptr{T}(C_NULL)
    Tp = want_posterior ? Array{T}(undef, D, D, B) : Ptr{T}(C_NULL)
    Ap = (want_posterior && pk != P_UPPER) ? Array{T}(undef, D, D, B) : Ptr{T}(C_NULL)
    lp = zeros(Cdouble, B)
    info = zeros(Int32, B)
    h = handle()
    check(h, posterior_ragged_call(h, T, MEM_HOST, layout, B, D, offsets, Xp, layout == COLVECS ? D : max(total, 1), yp, nk, sp, 1, pk, mwb, D,
                                   Lb, ldl, strideL, mw_post, D, Tp, D, D * D, Ap, D, D * D, lp, info))
    bad = findfirst(>(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))
    want_posterior || return [(lp[b], nothing, nothing, nothing) for b in 1:B]
    return [(lp[b], mw_post[:, b], Tp[:, :, b], Ap isa Ptr ? Ap : Ap[:, :, b]) for b in 1:B]
end

function logpdf_map(fxs::AbstractVector{<:FiniteGP}, ys::AbstractVector{<:AbstractVector{<:Real}})
    r = fused_many(fxs, ys, false)
    r === nothing ? map(logpdf, fxs, ys) : Float64[q[1] for q in r]
end

function posterior_map(fxs::AbstractVector{<:FiniteGP}, ys::AbstractVector{<:AbstractVector{<:Real}})
    r = fused_many(fxs, ys, true)
    r === nothing && return map(posterior, fxs, ys)
    map(fxs, r) do fx, (_, mw_post, Tp, Ap)
        blr0 = fx.f isa BasisFunctionRegressor ? fx.f.blr : fx.f
        post = BayesianLinearRegressor(mw_post, build_Λ(typeof(blr0.Λw), Tp, Ap))
        fx.f isa BasisFunctionRegressor ? BasisFunctionRegressor(post, fx.f.ϕ) : post
    end
end

# blr_posterior_multi_batched_* (include/blr_mi355x.h): B regressors with S target columns each (Y: N x S per regressor, ldY), one
# factor per regressor shared by its columns, a mean (D x S, ldmp) and an evidence (logpdf[b*stride_lp + s]) per column.  The arrays
# are host Arrays (MEM_HOST) or raw device pointers.
function posterior_multi_batched_call(h, ::Type{T}, memspace, layout, B, D, N, S, X, ldx, strideX, Y, ldY, strideY, nk, s, strides, pk,
                                      mw, stridemw, Lw, ldl, strideLw, mw_post, ldmp, stride_mwpost, Tp, ldt, strideT, Ap, ldlp, strideLp,
                                      lp, stride_lp, info) where {T<:Elt}
    GC.@preserve X Y s mw Lw mw_post Tp Ap lp info begin
        if T === Float64
            ccall((:blr_posterior_multi_batched_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Int32}),
                  h, memspace, layout, B, D, N, S, X, ldx, strideX, Y, ldY, strideY, nk, s, strides, pk, mw, stridemw,
                  Lw, ldl, strideLw, mw_post, ldmp, stride_mwpost, Tp, ldt, strideT, Ap, ldlp, strideLp, lp, stride_lp, info)
        else
            ccall((:blr_posterior_multi_batched_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Int32}),
                  h, memspace, layout, B, D, N, S, X, ldx, strideX, Y, ldY, strideY, nk, s, strides, pk, mw, stridemw,
                  Lw, ldl, strideLw, mw_post, ldmp, stride_mwpost, Tp, ldt, strideT, Ap, ldlp, strideLp, lp, stride_lp, info)
        end
    end
end

# logpdf(fx, Y::AbstractMatrix) under a map over data sets -> B x S matrix of column evidences.  Equal shapes (D, N, S, layout,
# isotropic or diagonal noise, prior kind, element type) make ONE blr_posterior_multi_batched_* call; anything else maps column by column.
function logpdf_map(fxs::AbstractVector{<:FiniteGP}, Ys::AbstractVector{<:AbstractMatrix{<:Real}})
    length(fxs) == length(Ys) || throw(DimensionMismatch("as many target matrices as finite regressors are needed"))
    B = length(fxs)
    B == 0 && return zeros(Float64, 0, 0)
    loop() = permutedims(reduce(hcat, [Float64[logpdf(fx, view(Y, :, j)) for j in axes(Y, 2)] for (fx, Y) in zip(fxs, Ys)]))
    any(fx -> fx.f isa BasisFunctionRegressor && fx.f.ϕ isa RandomFourierFeatures, fxs) && return loop()
    fbs = map(to_blr, fxs)
    xls, nzs, prs = map(fb -> xlayout(fb.x), fbs), map(fb -> noise(fb.Σy), fbs), map(fb -> prior(fb.f.Λw), fbs)
    (any(isnothing, xls) || any(isnothing, nzs) || any(isnothing, prs)) && return loop()
    X1, layout, _, D, N = xls[1]
    T = eltype(X1)
    S = size(Ys[1], 2)
    nk, pk = nzs[1][2], prs[1][2]
    (nk == DENSEN || D == 0 || S == 0) && return loop()
    alike = all(b -> eltype(xls[b][1]) === T && xls[b][2] == layout && xls[b][4] == D && xls[b][5] == N && nzs[b][2] == nk &&
                     prs[b][2] == pk && size(Ys[b]) == (N, S) && length(fbs[b].f.mw) == D, 1:B)
    alike || return loop()
    rows, cols = layout == COLVECS ? (D, N) : (N, D)
    Xb = Array{T}(undef, rows, cols, B)
    Yb = Array{T}(undef, N, S, B)
    ns = nk == ISOTROPIC ? 1 : N
    sb = Matrix{T}(undef, ns, B)
    mwb = Matrix{T}(undef, D, B)
    Lb = pk == P_DIAG ? Matrix{T}(undef, D, B) : Array{T}(undef, D, D, B)
    for b in 1:B
        copyto!(view(Xb, :, :, b), xls[b][1])
        Yb[:, :, b] .= Ys[b]
        sb[:, b] .= view(nzs[b][1], 1:ns)
        mwb[:, b] .= fbs[b].f.mw
        pk == P_DIAG ? (Lb[:, b] .= prs[b][1]) : copyto!(view(Lb, :, :, b), prs[b][1])
    end
    ldl, strideL = pk == P_DIAG ? (1, D) : (D, D * D)
    lp = zeros(Cdouble, S, B)
    info = zeros(Int32, B)
    h = handle()
    check(h, posterior_multi_batched_call(h, T, MEM_HOST, layout, B, D, N, S, Xb, rows, rows * cols, Yb, max(N, 1), N * S, nk, sb, ns, pk,
                                          mwb, D, Lb, ldl, strideL, Ptr{T}(C_NULL), D, D * S, Ptr{T}(C_NULL), D, D * D,
                                          Ptr{T}(C_NULL), D, D * D, lp, S, info))
    bad = findfirst(>(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))
    return permutedims(lp)
end

# The reference's own methods stay reachable after install_overrides! has replaced them: the fallbacks run in the world age
# recorded when this module was loaded (i.e. against the method tables as the reference defined them) -- no recursion.
const REF_WORLD = Ref{UInt}(0)
__init__() = (REF_WORLD[] = Base.get_world_counter(); nothing)
ref_call(f, args...) = Base.invoke_in_world(REF_WORLD[], f, args...)
REF_logpdf(fx, y) = ref_call(AbstractGPs.logpdf, fx, y)
REF_posterior(fx, y) = ref_call(AbstractGPs.posterior, fx, y)

# ---- marginal stream: reference :33, :40-43, :47 --------------------------------------------------------------
function mean_and_var(fx::FiniteGP; want_mean::Bool=true, want_var::Bool=true)
    fb = to_blr(fx)
    xl, nz, pr = xlayout(fb.x), noise(fb.Σy), prior(fb.f.Λw)
    (xl === nothing || nz === nothing || pr === nothing) && return ref_call(AbstractGPs.mean_and_var, fx)
    X, layout, ldx, D, N = xl
    T = eltype(X)
    mw = convert(Vector{T}, fb.f.mw)
    s, nk, _ = nz
    nk == DENSEN && ((s, nk) = (collect(diag(s)), DIAGONALN))                              # var adds diag(Σy) only (:43)
    Lw, pk, ldl = pr
    m = want_mean ? Vector{T}(undef, N) : Ptr{T}(C_NULL)
    v = want_var ? Vector{T}(undef, N) : Ptr{T}(C_NULL)
    info = Ref{Int32}(0)
    h = handle()
    rc = GC.@preserve X mw s Lw m v begin
        if T === Float64
            ccall((:blr_marginals_batched_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T},
                   Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ref{Int32}),
                  h, MEM_HOST, layout, 1, D, N, X, ldx, 0, nk, s, 0, pk, mw, 0, Lw, ldl, 0, m, N, v, N, info)
        else
            ccall((:blr_marginals_batched_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T},
                   Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ref{Int32}),
                  h, MEM_HOST, layout, 1, D, N, X, ldx, 0, nk, s, 0, pk, mw, 0, Lw, ldl, 0, m, N, v, N, info)
        end
    end
    check(h, rc)
    check(h, info[])
    return m, v
end
mean(fx::FiniteGP) = mean_and_var(fx; want_var=false)[1]
var(fx::FiniteGP) = mean_and_var(fx; want_mean=false)[2]
marginals(fx::FiniteGP) = ((m, v) = mean_and_var(fx); AbstractGPs.Normal.(m, sqrt.(v)))

# blr_marginals_multi_batched_* (include/blr_mi355x.h): S mean columns (M: D x S per regressor, ldm -- the mw_post block of
# blr_posterior_multi_batched_*) and ONE variance per input for B regressors.  The arrays are host Arrays (MEM_HOST) or raw device pointers.
function marginals_multi_batched_call(h, ::Type{T}, memspace, layout, B, D, N, S, X, ldx, strideX, nk, s, strides, pk, M, ldm, strideM,
                                      Lw, ldl, strideLw, m, ldmean, stridemean, v, stridevar, info) where {T<:Elt}
    GC.@preserve X s M Lw m v info begin
        if T === Float64
            ccall((:blr_marginals_multi_batched_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{Int32}),
                  h, memspace, layout, B, D, N, S, X, ldx, strideX, nk, s, strides, pk, M, ldm, strideM,
                  Lw, ldl, strideLw, m, ldmean, stridemean, v, stridevar, info)
        else
            ccall((:blr_marginals_multi_batched_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{Int32}),
                  h, memspace, layout, B, D, N, S, X, ldx, strideX, nk, s, strides, pk, M, ldm, strideM,
                  Lw, ldl, strideLw, m, ldmean, stridemean, v, stridevar, info)
        end
    end
end

# mean_and_var over the S column posteriors of a matrix target (posterior per column: they share the precision) at the inputs and
# noise of the FiniteGPs `fxs` (all S hold the same x and Σy): (mean N x S, var N) from one library call, :47 per column.
function mean_and_var(fxs::AbstractVector{<:FiniteGP})
    isempty(fxs) && throw(ArgumentError("at least one column posterior is needed"))
    fbs = map(to_blr, fxs)
    fb = fbs[1]
    all(f -> f.f.Λw === fb.f.Λw, fbs) || throw(ArgumentError("the columns must share one precision object"))
    xl, nz, pr = xlayout(fb.x), noise(fb.Σy), prior(fb.f.Λw)
    (xl === nothing || nz === nothing || pr === nothing) &&
        return (reduce(hcat, [mean_and_var(fx)[1] for fx in fxs]), mean_and_var(fxs[1])[2])
    X, layout, ldx, D, N = xl
    T = eltype(X)
    S = length(fbs)
    M = Matrix{T}(undef, D, S)
    for (j, f) in enumerate(fbs)
        M[:, j] .= f.f.mw
    end
    s, nk, _ = nz
    nk == DENSEN && ((s, nk) = (collect(diag(s)), DIAGONALN))                              # var adds diag(Σy) only (:43)
    Lw, pk, ldl = pr
    m = Matrix{T}(undef, N, S)
    v = Vector{T}(undef, N)
    info = zeros(Int32, 1)
    h = handle()
    check(h, marginals_multi_batched_call(h, T, MEM_HOST, layout, 1, D, N, S, X, ldx, 0, nk, s, 0, pk, M, max(D, 1), 0, Lw, ldl, 0,
                                          m, max(N, 1), 0, v, N, info))
    check(h, info[1])
    return m, v
end

# ---- full covariance: reference :35-38, :45 ----------------------------------------------------------------------
function mean_and_cov(fx::FiniteGP; want_mean::Bool=true)
    fb = to_blr(fx)
    xl, nz, pr = xlayout(fb.x), noise(fb.Σy), prior(fb.f.Λw)
    (xl === nothing || nz === nothing || pr === nothing) && return ref_call(AbstractGPs.mean_and_cov, fx)
    X, layout, ldx, D, N = xl
    T = eltype(X)
    mw = convert(Vector{T}, fb.f.mw)
    s, nk, lds = nz
    Lw, pk, ldl = pr
    m = want_mean ? Vector{T}(undef, N) : Ptr{T}(C_NULL)
    C = Matrix{T}(undef, N, N)
    info = Ref{Int32}(0)
    h = handle()
    rc = GC.@preserve X mw s Lw m C begin
        if T === Float64
            ccall((:blr_mean_and_cov_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Ptr{T}, Int64,
                   Ptr{T}, Ptr{T}, Int64, Ref{Int32}),
                  h, MEM_HOST, layout, D, N, X, ldx, nk, s, lds, pk, mw, Lw, ldl, m, C, N, info)
        else
            ccall((:blr_mean_and_cov_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Ptr{T}, Int64,
                   Ptr{T}, Ptr{T}, Int64, Ref{Int32}),
                  h, MEM_HOST, layout, D, N, X, ldx, nk, s, lds, pk, mw, Lw, ldl, m, C, N, info)
        end
    end
    check(h, rc)
    check(h, info[])
    return m, Symmetric(C)                                                                   # :37 Symmetric(α'α + Σy)
end
cov(fx::FiniteGP) = mean_and_cov(fx; want_mean=false)[2]

# blr_mean_and_cov_batched_* (include/blr_mi355x.h): mean[B][N] (may be C_NULL) and the full N x N covariance per regressor (C, ldc,
# strideC; may be C_NULL) for B regressors in one call, :33 / :35-38 / :45 under a map.  A stride of 0 shares an input (strideX = 0: one
# candidate set).  The arrays are host Arrays (MEM_HOST) or raw device pointers; one status per regressor lands in info.
function mean_and_cov_batched!(h, ::Type{T}, memspace, layout, B, D, N, X, ldx, strideX, nk, s, lds, strides, pk, mw, stridemw,
                               Lw, ldl, strideLw, m, stridemean, C, ldc, strideC, info) where {T<:Elt}
    GC.@preserve X s mw Lw m C info begin
        if T === Float64
            ccall((:blr_mean_and_cov_batched_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ptr{Int32}),
                  h, memspace, layout, B, D, N, X, ldx, strideX, nk, s, lds, strides, pk, mw, stridemw,
                  Lw, ldl, strideLw, m, stridemean, C, ldc, strideC, info)
        else
            ccall((:blr_mean_and_cov_batched_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ptr{Int32}),
                  h, memspace, layout, B, D, N, X, ldx, strideX, nk, s, lds, strides, pk, mw, stridemw,
                  Lw, ldl, strideLw, m, stridemean, C, ldc, strideC, info)
        end
    end
end

# ---- draws: reference :49-53 -- the RNG stream stays Julia's: Z1 = randn(rng, D, S) FIRST, then Z2 -------------
function rand(rng::AbstractRNG, fx::FiniteGP, samples::Int)
    fb = to_blr(fx)
    xl, nz, pr = xlayout(fb.x), noise(fb.Σy), prior(fb.f.Λw)
    (xl === nothing || nz === nothing || pr === nothing) && return ref_call(AbstractGPs.rand, rng, fx, samples)
    X, layout, ldx, D, N = xl
    T = eltype(X)
    mw = convert(Vector{T}, fb.f.mw)
    s, nk, lds = nz
    Lw, pk, ldl = pr
    Z1 = randn(rng, T, D, samples)       # reference :51
    Z2 = randn(rng, T, N, samples)       # reference :52
    Y = Matrix{T}(undef, N, samples)
    h = handle()
    rc = GC.@preserve X mw s Lw Z1 Z2 Y begin
        if nk == DENSEN
            if T === Float64
                ccall((:blr_rand_dense_noise_f64, LIB), Cint,
                      (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Ptr{T}, Int64,
                       Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64),
                      h, MEM_HOST, layout, D, N, samples, X, ldx, s, lds, pk, mw, Lw, ldl, Z1, D, Z2, N, Y, N)
            else
                ccall((:blr_rand_dense_noise_f32, LIB), Cint,
                      (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Ptr{T}, Int64,
                       Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64),
                      h, MEM_HOST, layout, D, N, samples, X, ldx, s, lds, pk, mw, Lw, ldl, Z1, D, Z2, N, Y, N)
            end
        elseif T === Float64
            ccall((:blr_rand_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Cint, Ptr{T}, Ptr{T}, Int64,
                   Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64),
                  h, MEM_HOST, layout, D, N, samples, X, ldx, nk, s, pk, mw, Lw, ldl, Z1, D, Z2, N, Y, N)
        else
            ccall((:blr_rand_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Cint, Ptr{T}, Ptr{T}, Int64,
                   Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64),
                  h, MEM_HOST, layout, D, N, samples, X, ldx, nk, s, pk, mw, Lw, ldl, Z1, D, Z2, N, Y, N)
        end
    end
    check(h, rc)
    return Y
end
rand(rng::AbstractRNG, fx::FiniteGP) = vec(rand(rng, fx, 1))

# ---- function-space samples: src/sampling_functions.jl:12-52 ------------------------------------------------------
function sample_weights(rng::AbstractRNG, blr::BayesianLinearRegressor, S::Int)
    pr = prior(blr.Λw)
    T = eltype(blr.mw)
    (pr === nothing || !(T <: Elt)) && return blr.mw .+ AbstractGPs._cholesky(blr.Λw).U \ randn(rng, length(blr.mw), S)
    D = length(blr.mw)
    Lw, pk, ldl = pr
    mw = convert(Vector{T}, blr.mw)
    Z = randn(rng, T, D, S)
    W = Matrix{T}(undef, D, S)
    h = handle()
    rc = GC.@preserve mw Lw Z W begin
        if T === Float64
            ccall((:blr_sample_weights_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64),
                  h, MEM_HOST, D, S, pk, mw, Lw, ldl, Z, D, W, D)
        else
            ccall((:blr_sample_weights_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64),
                  h, MEM_HOST, D, S, pk, mw, Lw, ldl, Z, D, W, D)
        end
    end
    check(h, rc)
    return W
end
const BLRLike = Union{BayesianLinearRegressor,BasisFunctionRegressor}
blr_and_mapping(b::BayesianLinearRegressor) = (b, identity)                               # sampling_functions.jl:51
blr_and_mapping(b::BasisFunctionRegressor) = (b.blr, b.ϕ)                                 # sampling_functions.jl:52
function rand(rng::AbstractRNG, b::BLRLike)                                               # sampling_functions.jl:27-31
    blr, ϕ = blr_and_mapping(b)
    BLRFunctionSample(vec(sample_weights(rng, blr, 1)), ϕ)
end
function rand(rng::AbstractRNG, b::BLRLike, dims::Dims)                                   # sampling_functions.jl:33-38
    blr, ϕ = blr_and_mapping(b)
    ws = sample_weights(rng, blr, prod(dims))
    reshape([BLRFunctionSample(collect(w), ϕ) for w in eachcol(ws)], dims)
end
rand(rng::AbstractRNG, b::BLRLike, d1::Integer, dims::Integer...) = rand(rng, b, Dims((d1, dims...)))
function rand!(rng::AbstractRNG, A::AbstractArray{<:BLRFunctionSample}, b::BLRLike)       # sampling_functions.jl:40-49
    blr, ϕ = blr_and_mapping(b)
    ws = sample_weights(rng, blr, length(A))
    for (i, w) in zip(eachindex(A), eachcol(ws))
        A[i] = BLRFunctionSample(collect(w), ϕ)
    end
    return A
end

# ---- Y = X'W for S given weight vectors (blr_apply_weights_*): a batch of function samples evaluated at the inputs,
#      sampling_functions.jl:16-18; `layout`, `D`, `N` describe X as the library reads it (see xlayout)
function apply_weights!(Y::Matrix{T}, X::Array{T}, layout::Integer, ldx::Integer, D::Integer, N::Integer, W::Matrix{T}) where {T<:Elt}
    S = size(W, 2)
    h = handle()
    rc = GC.@preserve X W Y begin
        if T === Float64
            ccall((:blr_apply_weights_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64),
                  h, MEM_HOST, layout, D, N, S, X, ldx, W, size(W, 1), Y, size(Y, 1))
        else
            ccall((:blr_apply_weights_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64),
                  h, MEM_HOST, layout, D, N, S, X, ldx, W, size(W, 1), Y, size(Y, 1))
        end
    end
    check(h, rc)
    return Y
end
"""
    evaluate(samples, x) -> Matrix (N x S)

Every function sample of `samples` (an array of `BLRFunctionSample`s drawn from ONE regressor, e.g. `rand(rng, f, S)`) at the
inputs `x`, in one pass over ϕ(x): column j is `samples[j](x)` (reference sampling_functions.jl:16-18).
"""
function evaluate(samples::AbstractArray{<:BLRFunctionSample}, x::AbstractVector)
    ϕx = first(samples).ϕ(x)
    xl = xlayout(ϕx)
    xl === nothing && return reduce(hcat, [smp(x) for smp in samples])
    X, layout, ldx, D, N = xl
    T = eltype(X)
    W = Matrix{T}(undef, D, length(samples))
    for (j, smp) in enumerate(samples)
        W[:, j] .= smp.w
    end
    return apply_weights!(Matrix{T}(undef, N, length(samples)), X, layout, ldx, D, N, W)
end

# ---- reverse-mode rule of rand(rng, fx, S) (README.md:56-60 differentiates it w.r.t. X, Σ, mw, Λw through Zygote) -------------
#   Y = X'W .+ sqrt.(s) .* Z2,  W = mw .+ U \ Z1   (reference :49-53), the draws held fixed:
#   W̄ = X Ȳ,  X̄ = W Ȳ',  m̄w = W̄ 1,  Ū = -triu(U'^-1 W̄ V'), V = U \ Z1,  s̄_n = Σ_s Ȳ[n,s] Z2[n,s] / (2 sqrt(s_n)).
# The two O(D N S) products are blr_apply_weights_* calls on re-interpreted layouts (the design matrix read with rows and
# columns swapped / the weights as the design matrix of an S-feature problem); the rest is D x D bookkeeping.
function ChainRulesCore.rrule(::typeof(rand), rng::AbstractRNG, fx::FiniteGP{<:BayesianLinearRegressor}, S::Int)
    xl, nz, pr = xlayout(fx.x), noise(fx.Σy), prior(fx.f.Λw)
    (xl === nothing || nz === nothing || pr === nothing || nz[2] == DENSEN) && error("rrule(rand): input types outside the device path")
    X, layout, ldx, D, N = xl
    T = eltype(X)
    mw = convert(Vector{T}, fx.f.mw)
    s, nk, _ = nz
    Lw, pk, ldl = pr
    rng0 = copy(rng)
    Y = rand(rng, fx, S)                        # consumes Z1 = randn(rng, T, D, S), then Z2 = randn(rng, T, N, S)
    Z1 = randn(rng0, T, D, S); Z2 = randn(rng0, T, N, S)
    U = UpperTriangular(Matrix{T}(AbstractGPs._cholesky(fx.f.Λw).U))
    V = U \ Z1
    W = mw .+ V
    function rand_pullback(Ȳ0)
        Ȳ = convert(Matrix{T}, ChainRulesCore.unthunk(Ȳ0))
        flip = layout == COLVECS ? ROWVECS : COLVECS
        W̄ = apply_weights!(Matrix{T}(undef, D, S), X, flip, ldx, N, D, Ȳ)                              # X Ȳ
        X̄ = if layout == COLVECS                                                                       # W Ȳ' as D x N
            apply_weights!(Matrix{T}(undef, D, N), W, ROWVECS, D, S, D, Matrix{T}(Ȳ'))
        else                                                                                            # ... as N x D
            apply_weights!(Matrix{T}(undef, N, D), Ȳ, ROWVECS, N, S, N, Matrix{T}(W'))
        end
        Ū = -triu(U' \ (W̄ * V'))
        Λ = fx.f.Λw
        dΛ = if Λ isa Diagonal
            Diagonal(diag(Ū) ./ (2 .* sqrt.(Λ.diag)))
        elseif Λ isa AbstractPDMat
            Tangent{typeof(Λ)}(chol = Tangent{typeof(Λ.chol)}(factors = UpperTriangular(Ū)))
        else
            M = tril(U * Ū'); M[diagind(M)] ./= 2                                                       # Φ(L' L̄), L = U'
            Ab = U \ (U \ M')'
            (Ab .+ Ab') ./ 2
        end
        sv = nk == DIAGONALN ? s : fill(s[1], N)
        s̄ = vec(sum(Ȳ .* Z2; dims=2)) ./ (2 .* sqrt.(sv))
        dΣ = fx.Σy isa Diagonal{<:Any,<:AbstractGPs.FillArrays.Fill} ?
             Tangent{typeof(fx.Σy)}(diag = Tangent{typeof(fx.Σy.diag)}(value = sum(s̄))) : Diagonal(s̄)
        df = Tangent{typeof(fx.f)}(mw = vec(sum(W̄; dims=2)), Λw = dΛ)
        dx = Tangent{typeof(fx.x)}(X = X̄)
        return NoTangent(), NoTangent(), Tangent{typeof(fx)}(f = df, x = dx, Σy = dΣ), NoTangent()
    end
    return Y, rand_pullback
end
ChainRulesCore.rrule(::typeof(AbstractGPs.rand), rng::AbstractRNG, fx::FiniteGP{<:BayesianLinearRegressor}, S::Int) =
    ChainRulesCore.rrule(rand, rng, fx, S)

# ---- value + gradient of the log marginal likelihood (the rule behind the ccall; SURVEY.md 8f rank 1) ---------------
# Returns (lp, dX, dy, ds, dmw, mw_post, Ainv).
function logpdf_grad(fb::FiniteGP{<:BayesianLinearRegressor}, y::AbstractVector{<:Real})
    xl, nz, pr = xlayout(fb.x), noise(fb.Σy), prior(fb.f.Λw)
    (xl === nothing || nz === nothing || pr === nothing || nz[2] == DENSEN) && error("logpdf_grad: input types outside the device path")
    X, layout, ldx, D, N = xl
    T = eltype(X)
    s, nk, _ = nz
    Lw, pk, ldl = pr
    yv = convert(Vector{T}, y); mw = convert(Vector{T}, fb.f.mw)
    dX = similar(X); dy = Vector{T}(undef, N); ds = Vector{T}(undef, N); dmw = Vector{T}(undef, D)
    mw′ = Vector{T}(undef, D); Ai = Matrix{T}(undef, D, D)
    lp = Ref{Cdouble}(0.0); info = Ref{Int32}(0)
    h = handle()
    rc = GC.@preserve X yv s Lw mw dX dy ds dmw mw′ Ai begin
        if T === Float64
            ccall((:blr_logpdf_grad_batched_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint,
                   Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ref{Cdouble}, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ref{Int32}),
                  h, MEM_HOST, layout, 1, D, N, X, ldx, 0, yv, 0, nk, s, 0, pk, mw, 0, Lw, ldl, 0, lp, dX, ldx, 0, dy, 0, ds, 0,
                  dmw, 0, mw′, 0, Ai, D, 0, info)
        else
            ccall((:blr_logpdf_grad_batched_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint,
                   Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ref{Cdouble}, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ref{Int32}),
                  h, MEM_HOST, layout, 1, D, N, X, ldx, 0, yv, 0, nk, s, 0, pk, mw, 0, Lw, ldl, 0, lp, dX, ldx, 0, dy, 0, ds, 0,
                  dmw, 0, mw′, 0, Ai, D, 0, info)
        end
    end
    check(h, rc)
    info[] > 0 && throw(PosDefException(info[]))
    return lp[], dX, dy, ds, dmw, mw′, Ai
end

# The reverse-mode rule (README.md:56-71: Zygote differentiates logpdf through the reference's Julia code; a ccall is opaque).
#   dL/dy = -S r, dL/dmw = X S r, dL/dX = (mw' r' - A^-1 X) S, dL/ds_n = -(s_n - r_n^2 - x_n'A^-1 x_n) / (2 s_n^2),
#   dL/dΛw = -(m m' + A^-1 - Λw^-1) / 2 with m = mw' - mw;  r = y - X'mw' (one call: blr_logpdf_grad_batched_*).
# Tangents mirror the primal structs: FiniteGP(f = BLR(mw, Λw), x = ColVecs/RowVecs(X), Σy).
function ChainRulesCore.rrule(::typeof(logpdf), fx::FiniteGP{<:BayesianLinearRegressor}, y::AbstractVector{<:Real})
    lp, dX, dy, ds, dmw, mw′, Ai = logpdf_grad(fx, y)
    function logpdf_pullback(Δ)
        δ = ChainRulesCore.unthunk(Δ)
        m = mw′ .- fx.f.mw
        Λ = fx.f.Λw
        dΛ = if Λ isa Diagonal
            Diagonal(δ .* (-(m .^ 2 .+ diag(Ai) .- inv.(Λ.diag)) ./ 2))
        elseif Λ isa AbstractPDMat
            # the reference reads a PDMat prior through its factor (_cholesky(Λw) = Λw.chol, :78), so the cotangent belongs to
            # chol.factors: Λw = U'U  =>  dU = U (G + G') with G = dL/dΛw = -(m m' + A^-1 - Λw^-1) / 2 (symmetric), upper part
            G = -(m * m' .+ Ai .- inv(Λ.chol)) ./ 2
            dU = UpperTriangular(δ .* (Matrix(Λ.chol.U) * (G .+ G')))
            Tangent{typeof(Λ)}(chol = Tangent{typeof(Λ.chol)}(factors = dU))
        else
            δ .* (-(m * m' .+ Ai .- inv(Matrix(Λ))) ./ 2)
        end
        dΣ = fx.Σy isa Diagonal{<:Any,<:AbstractGPs.FillArrays.Fill} ?
             Tangent{typeof(fx.Σy)}(diag = Tangent{typeof(fx.Σy.diag)}(value = δ * sum(ds))) : Diagonal(δ .* ds)
        df = Tangent{typeof(fx.f)}(mw = δ .* dmw, Λw = dΛ)
        dx = Tangent{typeof(fx.x)}(X = δ .* dX)                       # same container layout as the primal (D x N or N x D)
        return NoTangent(), Tangent{typeof(fx)}(f = df, x = dx, Σy = dΣ), δ .* dy
    end
    return lp, logpdf_pullback
end
ChainRulesCore.rrule(::typeof(AbstractGPs.logpdf), fx::FiniteGP{<:BayesianLinearRegressor}, y::AbstractVector{<:Real}) =
    ChainRulesCore.rrule(logpdf, fx, y)

# ---- logpdf(fx, Y::AbstractMatrix): shared-X multi-output evidence (AbstractGPs' column-wise fallback) ----------------
function logpdf(fx::FiniteBLR, Y::AbstractMatrix{<:Real})
    fb = to_blr(fx)
    xl, nz, pr = xlayout(fb.x), noise(fb.Σy), prior(fb.f.Λw)
    (xl === nothing || nz === nothing || pr === nothing || nz[2] == DENSEN) && return [logpdf(fb, y) for y in eachcol(Y)]
    X, layout, ldx, D, N = xl
    T = eltype(X)
    s, nk, _ = nz
    Lw, pk, ldl = pr
    size(Y, 1) == N || throw(DimensionMismatch("length(y) != size(fx.x.X, 2)"))
    S = size(Y, 2)
    Ym = convert(Matrix{T}, Y); mw = convert(Vector{T}, fb.f.mw)
    lp = Vector{Float64}(undef, S); info = Ref{Int32}(0)
    h = handle()
    rc = GC.@preserve X Ym s Lw mw lp begin
        if T === Float64
            ccall((:blr_logpdf_multi_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Cint, Ptr{T}, Ptr{T},
                   Int64, Ptr{Cdouble}, Ptr{T}, Int64, Ref{Int32}),
                  h, MEM_HOST, layout, D, N, S, X, ldx, Ym, N, nk, s, pk, mw, Lw, ldl, lp, C_NULL, D, info)
        else
            ccall((:blr_logpdf_multi_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Cint, Ptr{T}, Ptr{T},
                   Int64, Ptr{Cdouble}, Ptr{T}, Int64, Ref{Int32}),
                  h, MEM_HOST, layout, D, N, S, X, ldx, Ym, N, nk, s, pk, mw, Lw, ldl, lp, C_NULL, D, info)
        end
    end
    check(h, rc)
    info[] > 0 && throw(PosDefException(info[]))
    return lp
end

# ---- draws from many regressors in ONE call (blr_rand_batched_*): `[rand(rng, fx, S) for fx in fxs]` with the normals drawn in
# exactly that order (Z1_b, then Z2_b, problem by problem -- reference :51-52).  Problems the batched entry point does not take
# (mixed shapes / layouts / kinds, dense noise) are mapped one by one.  `info` of the first failing problem -> PosDefException.
function rand_batched_call(h, memspace, layout, B, D, N, S, X, ldx, strideX, nk, s, strides, pk, mw, stridemw, Lw, ldl, strideLw,
                           Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y, ldy, strideY, info, ::Type{T}) where {T<:Elt}
    if T === Float64
        ccall((:blr_rand_batched_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Int32}),
              h, memspace, layout, B, D, N, S, X, ldx, strideX, nk, s, strides, pk, mw, stridemw, Lw, ldl, strideLw,
              Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y, ldy, strideY, info)
    else
        ccall((:blr_rand_batched_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Int32}),
              h, memspace, layout, B, D, N, S, X, ldx, strideX, nk, s, strides, pk, mw, stridemw, Lw, ldl, strideLw,
              Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y, ldy, strideY, info)
    end
end

function rand_map(rng::AbstractRNG, fxs::AbstractVector{<:FiniteGP}, S::Int)
    B = length(fxs)
    B == 0 && return Matrix[]
    fbs = map(to_blr, fxs)
    xls, nzs, prs = map(fb -> xlayout(fb.x), fbs), map(fb -> noise(fb.Σy), fbs), map(fb -> prior(fb.f.Λw), fbs)
    one_by_one() = [rand(rng, fx, S) for fx in fxs]
    (any(isnothing, xls) || any(isnothing, nzs) || any(isnothing, prs)) && return one_by_one()
    X1, layout, ldx, D, N = xls[1]
    T = eltype(X1)
    nk, pk = nzs[1][2], prs[1][2]
    (nk == DENSEN || N == 0) && return one_by_one()
    same = all(b -> eltype(xls[b][1]) === T && xls[b][2] == layout && xls[b][4] == D && xls[b][5] == N && nzs[b][2] == nk &&
                    prs[b][2] == pk && length(fbs[b].f.mw) == D, 1:B)
    same || return one_by_one()
    rows, cols = layout == COLVECS ? (D, N) : (N, D)
    shared = all(b -> fbs[b].x === fbs[1].x, 1:B)               # one candidate set for the whole batch: passed once
    Xb = shared ? X1 : Array{T}(undef, rows, cols, B)
    if !shared
        for b in 1:B
            copyto!(view(Xb, :, :, b), xls[b][1])
        end
    end
    ns = nk == ISOTROPIC ? 1 : N
    sb, mwb = Matrix{T}(undef, ns, B), Matrix{T}(undef, D, B)
    Lb = pk == P_DIAG ? Matrix{T}(undef, D, B) : Array{T}(undef, D, D, B)
    Z1, Z2 = Array{T}(undef, D, S, B), Array{T}(undef, N, S, B)
    for b in 1:B
        sb[:, b] .= view(nzs[b][1], 1:ns)
        mwb[:, b] .= fbs[b].f.mw
        pk == P_DIAG ? (Lb[:, b] .= prs[b][1]) : copyto!(view(Lb, :, :, b), prs[b][1])
        Z1[:, :, b] .= randn(rng, T, D, S)                    # reference :51
        Z2[:, :, b] .= randn(rng, T, N, S)                    # reference :52
    end
    ldl, strideL = pk == P_DIAG ? (1, D) : (D, D * D)
    Y = Array{T}(undef, N, S, B)
    info = zeros(Int32, B)
    h = handle()
    rc = GC.@preserve Xb sb mwb Lb Z1 Z2 Y info rand_batched_call(h, MEM_HOST, layout, B, D, N, S, Xb, shared ? ldx : rows, shared ? 0 : rows * cols, nk,
                                                                  sb, ns, pk, mwb, D, Lb, ldl, strideL, Z1, D, D * S, Z2, N, N * S,
                                                                  Ptr{T}(C_NULL), D, D * S, Y, N, N * S, info, T)
    check(h, rc)
    bad = findfirst(>(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))
    return [Y[:, :, b] for b in 1:B]
end

# ---- device-resident batches: the form every throughput number is measured on ------------------------------------------
# A DeviceArray owns hipMalloc'd memory through the library's own helpers (no AMDGPU.jl needed); AMDGPU.jl users pass
# `Ptr{T}(pointer(roc_array))` instead.  Layout = Julia's: X is D x N x B column-major (regressor b at offset (b-1) D N).
mutable struct DeviceArray{T}
    ptr::Ptr{T}
    len::Int
    function DeviceArray{T}(len::Integer) where {T}
        p = Ref{Ptr{Cvoid}}(C_NULL)
        h = handle()
        check(h, ccall((:blr_device_alloc, LIB), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), h, len * sizeof(T), p))
        a = new{T}(Ptr{T}(p[]), len)
        finalizer(a -> ccall((:blr_device_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), handle(), a.ptr), a)
    end
end
# Run-time switches of this task's handle (A/B measurements and tests; the defaults are the measured best).  `key` with or
# without the BLR_MI355X_ prefix (include/blr_mi355x.h lists them); `value === nothing` restores the default.
function set_option!(key::AbstractString, value::Union{Nothing,AbstractString,Integer}=nothing)
    h = handle()
    v = value === nothing ? C_NULL : string(value)
    rc = ccall((:blr_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Cstring), h, key, v)
    rc == 0 || throw(ArgumentError("blr_set_option: unknown key or malformed value: $key = $value"))
    return nothing
end
# Which kernel family this task's most recent posterior / logpdf call ran on ("fused_i8_kernel", "fused_small_kernel<double, 8, 4>", ...).
last_route() = unsafe_string(ccall((:blr_last_route, LIB), Cstring, (Ptr{Cvoid},), handle()))
# Counters of this task's handle: "i8_regressors" (sent down the int8-sliced Gram route), "i8_handed_back" (of those, redone by the fp64
# kernel inside the same call: each cost two passes over its data -- heavy-tailed design matrices), "planes_redone" (fp32 updates at
# D > 128 whose sampled row scales did not hold: exact row maxima + the operand planes a second time), "workspace_bytes".
function get_stat(key::AbstractString)
    h = handle()
    v = Ref{Int64}(0)
    check(h, ccall((:blr_get_stat, LIB), Cint, (Ptr{Cvoid}, Cstring, Ref{Int64}), h, key, v))
    return v[]
end
reset_stats!() = (h = handle(); check(h, ccall((:blr_reset_stats, LIB), Cint, (Ptr{Cvoid},), h)); nothing)
# Give the handle's workspace, feature and side buffers back to the allocator (they are re-created by the next call that needs them).
release_workspace!() = (h = handle(); check(h, ccall((:blr_release_workspace, LIB), Cint, (Ptr{Cvoid},), h)); nothing)

function upload(a::Array{T}) where {T}
    d = DeviceArray{T}(length(a))
    h = handle()
    GC.@preserve a check(h, ccall((:blr_memcpy_h2d, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), h, d.ptr, a, sizeof(a)))
    d
end
function download!(a::Array{T}, d::DeviceArray{T}) where {T}
    h = handle()
    GC.@preserve a check(h, ccall((:blr_memcpy_d2h, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), h, a, d.ptr, sizeof(a)))
    a
end

"""
    posterior_ragged!(mw_post, T_post, logpdf, info, X, offsets, y, s, mw, Λdiag; D, isotropic)

B = length(offsets) - 1 regressors with UNEQUAL observation counts in ONE launch (D ≤ 128), everything device resident except
`offsets` (a host `Vector{Int64}`, zero based, B + 1 non-decreasing entries): regressor b owns the columns offsets[b]+1:offsets[b+1]
of X (D×offsets[end], ColVecs) and the same entries of y; s holds B variances (`isotropic`) or offsets[end]; mw is D×B, Λdiag the
D diagonal entries of a prior precision shared by the batch; outputs as `posterior_batched!`.  Reference semantics per regressor:
`:55-69` under a map over fxs of different lengths.
"""
function posterior_ragged!(mw_post::DeviceArray{T}, T_post::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                           X::DeviceArray{T}, offsets::Vector{Int64}, y::DeviceArray{T}, s::DeviceArray{T}, mw::DeviceArray{T},
                           Λdiag::DeviceArray{T}; D::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    B = length(offsets) - 1
    check(h, posterior_ragged_call(h, T, MEM_DEVICE, COLVECS, B, D, offsets, X.ptr, D, y.ptr, isotropic ? ISOTROPIC : DIAGONALN, s.ptr,
                                   isotropic ? 1 : 0, P_DIAG, mw.ptr, D, Λdiag.ptr, 1, 0, mw_post.ptr, D, T_post.ptr, D, D * D,
                                   Ptr{T}(C_NULL), D, D * D, lp.ptr, info.ptr))
    return nothing
end

function marginals_ragged_call(h, ::Type{T}, memspace, layout, B, D, offsets::Vector{Int64}, X, ldx, nk, s, strides, pk, mw, stridemw,
                               Lw, ldl, strideLw, m, v, info) where {T<:Elt}
    GC.@preserve offsets X s mw Lw m v info begin
        if T === Float64
            ccall((:blr_marginals_ragged_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, nk, s, strides, pk, mw, stridemw, Lw, ldl, strideLw, m, v, info)
        else
            ccall((:blr_marginals_ragged_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, nk, s, strides, pk, mw, stridemw, Lw, ldl, strideLw, m, v, info)
        end
    end
end

function loo_ragged_call(h, ::Type{T}, memspace, layout, B, D, offsets::Vector{Int64}, X, ldx, y, nk, s, strides, mw, stridemw,
                         Tf, ldt, strideT, lm, lv, ll, tot, info) where {T<:Elt}
    GC.@preserve offsets X y s mw Tf lm lv ll tot info begin
        if T === Float64
            ccall((:blr_loo_ragged_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, lm, lv, ll, tot, info)
        else
            ccall((:blr_loo_ragged_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, lm, lv, ll, tot, info)
        end
    end
end

"""
    marginals_ragged!(mean, var, info, X, offsets, s, mw_post, T_post; D, isotropic)

Predictions of B = length(offsets) - 1 regressors with UNEQUAL observation counts at their own inputs, from the state
`posterior_ragged!` leaves, in one call (D ≤ 128: one workgroup per work item, a long regressor is spread over the chip); `offsets`
as there.  mean and var are packed as the inputs are (offsets[end] entries); info B (Int32).  Reference semantics per regressor:
`:33`, `:40-43`, `:47` under a map over fxs of different lengths.
"""
function marginals_ragged!(m::DeviceArray{T}, v::DeviceArray{T}, info::DeviceArray{Int32}, X::DeviceArray{T}, offsets::Vector{Int64},
                           s::DeviceArray{T}, mw_post::DeviceArray{T}, T_post::DeviceArray{T}; D::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    B = length(offsets) - 1
    check(h, marginals_ragged_call(h, T, MEM_DEVICE, COLVECS, B, D, offsets, X.ptr, D, isotropic ? ISOTROPIC : DIAGONALN, s.ptr,
                                   isotropic ? 1 : 0, P_UPPER, mw_post.ptr, D, T_post.ptr, D, D * D, m.ptr, v.ptr, info.ptr))
    return nothing
end

"""
    loo_ragged!(loo_mean, loo_var, loo_logpdf, loo_total, info, X, offsets, y, s, mw_post, T_post; D, isotropic)

Exact leave-one-out predictives of the observations the states of `posterior_ragged!` contain, for B = length(offsets) - 1
regressors with UNEQUAL observation counts in one call; the per-observation outputs are packed as the inputs are, loo_total and
info have B entries.  Reference semantics: `:55-58` for each held-out point given the rest, under a map over fxs of different
lengths.
"""
function loo_ragged!(lm::DeviceArray{T}, lv::DeviceArray{T}, ll::DeviceArray{Float64}, tot::DeviceArray{Float64}, info::DeviceArray{Int32},
                     X::DeviceArray{T}, offsets::Vector{Int64}, y::DeviceArray{T}, s::DeviceArray{T}, mw_post::DeviceArray{T},
                     T_post::DeviceArray{T}; D::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    B = length(offsets) - 1
    check(h, loo_ragged_call(h, T, MEM_DEVICE, COLVECS, B, D, offsets, X.ptr, D, y.ptr, isotropic ? ISOTROPIC : DIAGONALN, s.ptr,
                             isotropic ? 1 : 0, mw_post.ptr, D, T_post.ptr, D, D * D, lm.ptr, lv.ptr, ll.ptr, tot.ptr, info.ptr))
    return nothing
end

# blr_update_factor_ragged_* / blr_downdate_factor_ragged_* (include/blr_mi355x.h): resident states that received unequal numbers
# of observations, revised in place in one call; `down`: forget
function revise_ragged_call(h, ::Type{T}, down::Bool, memspace, layout, B, D, offsets::Vector{Int64}, X, ldx, y, nk, s, strides, mw,
                            stridemw, Tf, ldt, strideT, lp, info) where {T<:Elt}
    GC.@preserve offsets X y s mw Tf lp info begin
        if T === Float64 && !down
            ccall((:blr_update_factor_ragged_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, lp, info)
        elseif T === Float64
            ccall((:blr_downdate_factor_ragged_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, lp, info)
        elseif !down
            ccall((:blr_update_factor_ragged_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, lp, info)
        else
            ccall((:blr_downdate_factor_ragged_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, lp, info)
        end
    end
end

"""
    update_factor_ragged!(mw, T_factor, logpdf, info, X, offsets, y, s; D, isotropic)
    downdate_factor_ragged!(mw, T_factor, logpdf, info, X, offsets, y, s; D, isotropic)

Condition (or forget) B = length(offsets) - 1 RESIDENT states in place, each on its own number of observations -- none included --
in one call: mw is D×B, T_factor D×D×B (upper factors), X D×offsets[end] (ColVecs), y packed likewise, s holds B variances
(`isotropic`) or offsets[end]; `offsets` as `posterior_ragged!` takes it.  logpdf (B, Float64): log p(y_b | state before) for the
update, log p(y_b | state after) for the downdate, 0 for a regressor without observations; info (B, Int32): a state whose info is
not 0 is untouched.  Reference semantics per regressor: "repeated conditioning", test/bayesian_linear_regression.jl:49-70.
"""
function update_factor_ragged!(mw::DeviceArray{T}, Tf::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                               X::DeviceArray{T}, offsets::Vector{Int64}, y::DeviceArray{T}, s::DeviceArray{T}; D::Int,
                               isotropic::Bool) where {T<:Elt}
    h = handle()
    B = length(offsets) - 1
    check(h, revise_ragged_call(h, T, false, MEM_DEVICE, COLVECS, B, D, offsets, X.ptr, D, y.ptr, isotropic ? ISOTROPIC : DIAGONALN, s.ptr,
                                isotropic ? 1 : 0, mw.ptr, D, Tf.ptr, D, D * D, lp.ptr, info.ptr))
    return nothing
end

function downdate_factor_ragged!(mw::DeviceArray{T}, Tf::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                                 X::DeviceArray{T}, offsets::Vector{Int64}, y::DeviceArray{T}, s::DeviceArray{T}; D::Int,
                                 isotropic::Bool) where {T<:Elt}
    h = handle()
    B = length(offsets) - 1
    check(h, revise_ragged_call(h, T, true, MEM_DEVICE, COLVECS, B, D, offsets, X.ptr, D, y.ptr, isotropic ? ISOTROPIC : DIAGONALN, s.ptr,
                                isotropic ? 1 : 0, mw.ptr, D, Tf.ptr, D, D * D, lp.ptr, info.ptr))
    return nothing
end

function kfold_ragged_call(h, ::Type{T}, memspace, layout, B, D, offsets::Vector{Int64}, F, X, ldx, y, nk, s, strides, mw, stridemw,
                           Tf, ldt, strideT, km, kv, kl, tot, info) where {T<:Elt}
    GC.@preserve offsets X y s mw Tf km kv kl tot info begin
        if T === Float64
            ccall((:blr_kfold_ragged_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Int64, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, F, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, km, kv, kl, tot, info)
        else
            ccall((:blr_kfold_ragged_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Int64, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, F, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, km, kv, kl, tot, info)
        end
    end
end

"""
    kfold_ragged_fold_offsets(offsets, F) -> Vector{Int64}

`fold_offsets` of `kfold_ragged!`: fold f of regressor b is entry `fold_offsets[b] + f` (0-based) of kf_logpdf, which holds
`fold_offsets[end]` entries.  Host arithmetic only (`blr_kfold_ragged_fold_offsets`).
"""
function kfold_ragged_fold_offsets(offsets::Vector{Int64}, F::Integer)
    B = length(offsets) - 1
    fo = Vector{Int64}(undef, B + 1)
    rc = ccall((:blr_kfold_ragged_fold_offsets, LIB), Cint, (Int64, Ptr{Int64}, Int64, Ptr{Int64}), B, offsets, F, fo)
    rc == 0 || error("blr_kfold_ragged_fold_offsets: argument $(-rc)")
    return fo
end

"""
    kfold_ragged!(kf_mean, kf_var, kf_logpdf, kf_total, info, X, offsets, y, s, mw_post, T_post; D, F, isotropic)

Exact leave-fold-out (K-fold) predictives of the observations the states of `posterior_ragged!` contain, for B = length(offsets) - 1
regressors with UNEQUAL observation counts in one call: regressor b has the contiguous folds of F ≤ 64 observations of its own
slice.  kf_mean and kf_var are packed as the inputs are, kf_logpdf by folds (`kfold_ragged_fold_offsets`), kf_total and info have B
entries.  Reference semantics: `:55-58` for each held-out fold given the rest, under a map over fxs of different lengths.
"""
function kfold_ragged!(km::DeviceArray{T}, kv::DeviceArray{T}, kl::DeviceArray{Float64}, tot::DeviceArray{Float64}, info::DeviceArray{Int32},
                       X::DeviceArray{T}, offsets::Vector{Int64}, y::DeviceArray{T}, s::DeviceArray{T}, mw_post::DeviceArray{T},
                       T_post::DeviceArray{T}; D::Int, F::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    B = length(offsets) - 1
    check(h, kfold_ragged_call(h, T, MEM_DEVICE, COLVECS, B, D, offsets, F, X.ptr, D, y.ptr, isotropic ? ISOTROPIC : DIAGONALN, s.ptr,
                               isotropic ? 1 : 0, mw_post.ptr, D, T_post.ptr, D, D * D, km.ptr, kv.ptr, kl.ptr, tot.ptr, info.ptr))
    return nothing
end

function kfold_large_ragged_call(h, ::Type{T}, memspace, layout, B, D, offsets::Vector{Int64}, fold_sizes::Vector{Int64}, X, ldx, y, nk, s,
                                 strides, mw, stridemw, Tf, ldt, strideT, km, kv, kl, tot, info) where {T<:Elt}
    GC.@preserve offsets fold_sizes X y s mw Tf km kv kl tot info begin
        if T === Float64
            ccall((:blr_kfold_large_ragged_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, fold_sizes, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, km, kv, kl, tot, info)
        else
            ccall((:blr_kfold_large_ragged_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                  h, memspace, layout, B, D, offsets, fold_sizes, X, ldx, y, nk, s, strides, mw, stridemw, Tf, ldt, strideT, km, kv, kl, tot, info)
        end
    end
end

"""
    kfold_large_ragged_fold_sizes(offsets, K) -> Vector{Int64}

`F_b = max(1, ceil(N_b / K))`: the fold sizes of K folds per regressor (`blr_kfold_large_ragged_fold_sizes`; host arithmetic only).
"""
function kfold_large_ragged_fold_sizes(offsets::Vector{Int64}, K::Integer)
    B = length(offsets) - 1
    fs = Vector{Int64}(undef, B)
    rc = ccall((:blr_kfold_large_ragged_fold_sizes, LIB), Cint, (Int64, Ptr{Int64}, Int64, Ptr{Int64}), B, offsets, K, fs)
    rc == 0 || error("blr_kfold_large_ragged_fold_sizes: argument $(-rc)")
    return fs
end

"""
    kfold_large_ragged_fold_offsets(offsets, fold_sizes) -> Vector{Int64}

`fold_offsets` of `kfold_large_ragged!`: fold f of regressor b is entry `fold_offsets[b] + f` (0-based) of kf_logpdf, which holds
`fold_offsets[end]` entries.  Host arithmetic only (`blr_kfold_large_ragged_fold_offsets`).
"""
function kfold_large_ragged_fold_offsets(offsets::Vector{Int64}, fold_sizes::Vector{Int64})
    B = length(offsets) - 1
    fo = Vector{Int64}(undef, B + 1)
    rc = ccall((:blr_kfold_large_ragged_fold_offsets, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), B, offsets, fold_sizes, fo)
    rc == 0 || error("blr_kfold_large_ragged_fold_offsets: argument $(-rc)")
    return fo
end

"""
    kfold_large_ragged!(kf_mean, kf_var, kf_logpdf, kf_total, info, X, offsets, fold_sizes, y, s, mw_post, T_post; D, isotropic)

Exact leave-fold-out (K-fold) predictives for LARGE folds of the observations the states of `posterior_ragged!` contain, for
B = length(offsets) - 1 regressors with UNEQUAL observation counts in one call: regressor b has the contiguous folds of
`fold_sizes[b]` observations of its own slice (`kfold_large_ragged_fold_sizes` for K folds each); D ≤ 128.  kf_mean and kf_var are
packed as the inputs are, kf_logpdf by folds (`kfold_large_ragged_fold_offsets`), kf_total and info have B entries.  Reference
semantics: `:55-58` for each held-out fold given the rest, under a map over fxs of different lengths.
"""
function kfold_large_ragged!(km::DeviceArray{T}, kv::DeviceArray{T}, kl::DeviceArray{Float64}, tot::DeviceArray{Float64}, info::DeviceArray{Int32},
                             X::DeviceArray{T}, offsets::Vector{Int64}, fold_sizes::Vector{Int64}, y::DeviceArray{T}, s::DeviceArray{T},
                             mw_post::DeviceArray{T}, T_post::DeviceArray{T}; D::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    B = length(offsets) - 1
    length(fold_sizes) == B || error("fold_sizes must have B = $B entries")
    check(h, kfold_large_ragged_call(h, T, MEM_DEVICE, COLVECS, B, D, offsets, fold_sizes, X.ptr, D, y.ptr, isotropic ? ISOTROPIC : DIAGONALN,
                                     s.ptr, isotropic ? 1 : 0, mw_post.ptr, D, T_post.ptr, D, D * D, km.ptr, kv.ptr, kl.ptr, tot.ptr, info.ptr))
    return nothing
end

"""
    posterior_multi_batched!(mw_post, T_post, logpdf, info, X, Y, s, mw, Λdiag; D, N, S, B, isotropic)

B regressors with S target columns each in ONE call (D ≤ 128: column 0 through the batched update, the other columns in one more
launch), everything device resident: X is D×N×B (ColVecs), Y N×S×B, s one variance per regressor (`isotropic`) or N×B, mw D×B, Λdiag
the D diagonal entries of a prior precision shared by the batch; outputs mw_post D×S×B, T_post D×D×B (ONE upper factor per
regressor, shared by its columns), logpdf S×B (Float64), info B (Int32).  Reference semantics per column: `:55-69` under a map over
fxs with matrix targets.
"""
function posterior_multi_batched!(mw_post::DeviceArray{T}, T_post::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                                  X::DeviceArray{T}, Y::DeviceArray{T}, s::DeviceArray{T}, mw::DeviceArray{T}, Λdiag::DeviceArray{T};
                                  D::Int, N::Int, S::Int, B::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    check(h, posterior_multi_batched_call(h, T, MEM_DEVICE, COLVECS, B, D, N, S, X.ptr, D, D * N, Y.ptr, max(N, 1), N * S,
                                          isotropic ? ISOTROPIC : DIAGONALN, s.ptr, isotropic ? 1 : N, P_DIAG, mw.ptr, D, Λdiag.ptr, 1, 0,
                                          mw_post.ptr, D, D * S, T_post.ptr, D, D * D, Ptr{T}(C_NULL), D, D * D, lp.ptr, S, info.ptr))
    return nothing
end

"""
    marginals_multi_batched!(mean, var, info, X, M, s, T_post; D, N, S, B, isotropic)

Predictions from the state `posterior_multi_batched!` leaves, in ONE call, everything device resident: X is D×N×B (ColVecs), M the
D×S×B posterior means (`mw_post`), T_post the D×D×B upper factors, s one variance per regressor (`isotropic`) or N×B; outputs mean
N×S×B and var N×B (one variance per input: it does not depend on the column), info B (Int32).  Reference semantics per column:
`:33`, `:40-43`, `:47` under a map over fxs whose regressors come from matrix targets.
"""
function marginals_multi_batched!(m::DeviceArray{T}, v::DeviceArray{T}, info::DeviceArray{Int32}, X::DeviceArray{T}, M::DeviceArray{T},
                                  s::DeviceArray{T}, T_post::DeviceArray{T}; D::Int, N::Int, S::Int, B::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    check(h, marginals_multi_batched_call(h, T, MEM_DEVICE, COLVECS, B, D, N, S, X.ptr, D, D * N, isotropic ? ISOTROPIC : DIAGONALN,
                                          s.ptr, isotropic ? 1 : N, P_UPPER, M.ptr, D, D * S, T_post.ptr, D, D * D, m.ptr, max(N, 1),
                                          N * S, v.ptr, N, info.ptr))
    return nothing
end

"""
    posterior_batched!(mw_post, T_post, logpdf, info, X, y, s, mw, Λdiag; D, N, B, isotropic)

B independent regressors in ONE launch, everything device resident (`DeviceArray`s): X is D×N×B, y N×B, s one variance
(`isotropic`) or N×B, mw D×B, Λdiag the D diagonal entries of a prior precision shared by the batch; outputs mw_post D×B,
T_post D×D×B (upper factors), logpdf B (Float64), info B (Int32).  Reference semantics per regressor: `:55-69`.
"""
function posterior_batched!(mw_post::DeviceArray{T}, T_post::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                            X::DeviceArray{T}, y::DeviceArray{T}, s::DeviceArray{T}, mw::DeviceArray{T}, Λdiag::DeviceArray{T};
                            D::Int, N::Int, B::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    rc = if T === Float64
        ccall((:blr_posterior_batched_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T},
               Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, isotropic ? 0 : N, P_DIAG, mw.ptr, D,
              Λdiag.ptr, 1, 0, mw_post.ptr, D, T_post.ptr, D, D * D, Ptr{T}(C_NULL), D, D * D, lp.ptr, info.ptr)
    else
        ccall((:blr_posterior_batched_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T},
               Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, isotropic ? 0 : N, P_DIAG, mw.ptr, D,
              Λdiag.ptr, 1, 0, mw_post.ptr, D, T_post.ptr, D, D * D, Ptr{T}(C_NULL), D, D * D, lp.ptr, info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    update_factor!(mw, T, logpdf, info, X, y, s; D, k, B, isotropic)

Condition B device-resident posterior states IN PLACE on k further observations each -- the "repeated conditioning" of
reference `test/bayesian_linear_regression.jl:49-70` without going back through a D×D precision (`:93`, `:72-89`):
mw is D×B, T D×D×B (upper factors, exactly what `posterior_batched!` wrote), X D×k×B, y k×B, s one variance (`isotropic`) or
k×B.  `logpdf[b]` = log p(y_b | state before the call) -- the evidence increment of the chain rule.
"""
function update_factor!(mw::DeviceArray{T}, Tf::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                        X::DeviceArray{T}, y::DeviceArray{T}, s::DeviceArray{T}; D::Int, k::Int, B::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    rc = if T === Float64
        ccall((:blr_update_factor_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, k, X.ptr, D, D * k, y.ptr, k, nk, s.ptr, isotropic ? 0 : k, mw.ptr, D, Tf.ptr, D, D * D,
              lp.ptr, info.ptr)
    else
        ccall((:blr_update_factor_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, k, X.ptr, D, D * k, y.ptr, k, nk, s.ptr, isotropic ? 0 : k, mw.ptr, D, Tf.ptr, D, D * D,
              lp.ptr, info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    downdate_factor!(mw, T, logpdf, info, X, y, s; D, k, B, isotropic)

The inverse of `update_factor!`: remove k observations from each of B device-resident posterior states IN PLACE (a sliding
window, retracted records), undoing the "repeated conditioning" of reference `test/bayesian_linear_regression.jl:49-70`.
Operands exactly as for `update_factor!`.  `logpdf[b]` = log p(y_b | state after the call), the density of the removed data
given what remains (reference `src/bayesian_linear_regression.jl:55-58`; at k = 1 the leave-one-out density).  info[b] > 0:
a bad factor, a bad variance, or a removal that leaves no positive definite precision; that state is left untouched.
"""
function downdate_factor!(mw::DeviceArray{T}, Tf::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                          X::DeviceArray{T}, y::DeviceArray{T}, s::DeviceArray{T}; D::Int, k::Int, B::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    rc = if T === Float64
        ccall((:blr_downdate_factor_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, k, X.ptr, D, D * k, y.ptr, k, nk, s.ptr, isotropic ? 0 : k, mw.ptr, D, Tf.ptr, D, D * D,
              lp.ptr, info.ptr)
    else
        ccall((:blr_downdate_factor_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, k, X.ptr, D, D * k, y.ptr, k, nk, s.ptr, isotropic ? 0 : k, mw.ptr, D, Tf.ptr, D, D * D,
              lp.ptr, info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    update_multi_factor!(M, T, logpdf, info, X, Y, s; D, k, S, B, isotropic)

Condition B device-resident MULTI-OUTPUT states IN PLACE on k further observations with S targets each: M is D×S×B (the means
`posterior_multi_batched!` wrote), T D×D×B (ONE upper factor per regressor), X D×k×B, Y k×S×B, s one variance (`isotropic`) or
k×B.  The factor work is done once per regressor (column 1 is `update_factor!`, bit for bit); `logpdf[c, b]` (S×B) =
log p(Y[:, c, b] | state before the call).  A regressor with `info[b] != 0` keeps its state and gets NaN evidences.
"""
function update_multi_factor!(M::DeviceArray{T}, Tf::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                              X::DeviceArray{T}, Y::DeviceArray{T}, s::DeviceArray{T}; D::Int, k::Int, S::Int, B::Int,
                              isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    rc = if T === Float64
        ccall((:blr_update_multi_factor_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, k, S, X.ptr, D, D * k, Y.ptr, max(k, 1), k * S, nk, s.ptr, isotropic ? 0 : k, M.ptr, D, D * S,
              Tf.ptr, D, D * D, lp.ptr, S, info.ptr)
    else
        ccall((:blr_update_multi_factor_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, k, S, X.ptr, D, D * k, Y.ptr, max(k, 1), k * S, nk, s.ptr, isotropic ? 0 : k, M.ptr, D, D * S,
              Tf.ptr, D, D * D, lp.ptr, S, info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    downdate_multi_factor!(M, T, logpdf, info, X, Y, s; D, k, S, B, isotropic)

The inverse of `update_multi_factor!`: remove k observations with S targets each from B device-resident multi-output states IN
PLACE.  Operands exactly as for `update_multi_factor!`; `logpdf[c, b]` = log p(Y[:, c, b] | state after the call), the contract of
`downdate_factor!` per column, and its status codes.
"""
function downdate_multi_factor!(M::DeviceArray{T}, Tf::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                              X::DeviceArray{T}, Y::DeviceArray{T}, s::DeviceArray{T}; D::Int, k::Int, S::Int, B::Int,
                              isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    rc = if T === Float64
        ccall((:blr_downdate_multi_factor_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, k, S, X.ptr, D, D * k, Y.ptr, max(k, 1), k * S, nk, s.ptr, isotropic ? 0 : k, M.ptr, D, D * S,
              Tf.ptr, D, D * D, lp.ptr, S, info.ptr)
    else
        ccall((:blr_downdate_multi_factor_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, k, S, X.ptr, D, D * k, Y.ptr, max(k, 1), k * S, nk, s.ptr, isotropic ? 0 : k, M.ptr, D, D * S,
              Tf.ptr, D, D * D, lp.ptr, S, info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    loo!(lmean, lvar, llogpdf, total, info, X, y, s, mw, T; D, N, B, isotropic)

Exact leave-one-out predictives of the N observations each of B device-resident states contains (`blr_loo_batched_*`): for
every n the predictive of y_n given all the other data -- what a `downdate_factor!` of observation n alone (followed by an
`update_factor!` to put it back) reports, and reference `src/bayesian_linear_regression.jl:55-58` applied to the held-out
point -- from one marginal pass, the states untouched.  Operands as for `downdate_factor!` with k = N; lmean, lvar (element
type) and llogpdf (Float64) are N×B or `nothing`, total (Float64, Σ_n llogpdf in a fixed order) B or `nothing`.  A
leverage within rounding of 1 gives NaN (`get_stat("loo_degenerate")` counts them); info[b] > 0: a bad factor, else a bad
variance, and that state's outputs are left untouched.
"""
function loo!(lm::Union{Nothing,DeviceArray{T}}, lv::Union{Nothing,DeviceArray{T}}, ll::Union{Nothing,DeviceArray{Float64}},
              total::Union{Nothing,DeviceArray{Float64}}, info::DeviceArray{Int32}, X::DeviceArray{T}, y::DeviceArray{T},
              s::DeviceArray{T}, mw::DeviceArray{T}, Tf::DeviceArray{T}; D::Int, N::Int, B::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : a.ptr
    dptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : a.ptr
    rc = if T === Float64
        ccall((:blr_loo_batched_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, isotropic ? 0 : N, mw.ptr, D, Tf.ptr, D, D * D,
              ptr(lm), N, ptr(lv), N, dptr(ll), N, dptr(total), info.ptr)
    else
        ccall((:blr_loo_batched_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, isotropic ? 0 : N, mw.ptr, D, Tf.ptr, D, D * D,
              ptr(lm), N, ptr(lv), N, dptr(ll), N, dptr(total), info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    kfold!(kmean, kvar, klogpdf, total, info, X, y, s, mw, T; D, N, F, B, isotropic)

Exact leave-fold-out (K-fold) predictives of the N observations each of B device-resident states contains
(`blr_kfold_batched_*`), for contiguous folds of F ≤ 64 observations: what a `downdate_factor!` of the fold, a prediction at
its inputs and an `update_factor!` to put it back report, the states untouched.  Operands as for `loo!`; kmean, kvar (element
type) are N×B or `nothing`, klogpdf (Float64, the JOINT log density of each fold) is cld(N, F)×B or `nothing`, total
(Float64, Σ_f klogpdf in a fixed order) B or `nothing`.  A fold the state does not contain gives NaN
(`get_stat("kfold_degenerate")` counts it once); info[b] > 0: a bad factor, else a bad variance, and that state's outputs
are left untouched.  D > 128 synchronises.
"""
function kfold!(km::Union{Nothing,DeviceArray{T}}, kv::Union{Nothing,DeviceArray{T}}, kl::Union{Nothing,DeviceArray{Float64}},
                total::Union{Nothing,DeviceArray{Float64}}, info::DeviceArray{Int32}, X::DeviceArray{T}, y::DeviceArray{T},
                s::DeviceArray{T}, mw::DeviceArray{T}, Tf::DeviceArray{T}; D::Int, N::Int, F::Int, B::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    nf = cld(N, F)
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : a.ptr
    dptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : a.ptr
    rc = if T === Float64
        ccall((:blr_kfold_batched_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, F, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, isotropic ? 0 : N, mw.ptr, D, Tf.ptr, D, D * D,
              ptr(km), N, ptr(kv), N, dptr(kl), nf, dptr(total), info.ptr)
    else
        ccall((:blr_kfold_batched_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, F, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, isotropic ? 0 : N, mw.ptr, D, Tf.ptr, D, D * D,
              ptr(km), N, ptr(kv), N, dptr(kl), nf, dptr(total), info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    kfold_large!(kmean, kvar, klogpdf, total, info, X, y, s, mw, T; D, N, F, B, isotropic)

The leave-fold-out predictives of `kfold!` for LARGE folds (`blr_kfold_large_batched_*`): any F ≥ 1 with cld(N, F) ≤ 1024, so the
K = 5 or 10 folds of N / K observations people cross-validate with; D ≤ 128.  The fold is removed in weight space: one D×D
factorisation of `T'T − X_f S_f⁻¹ X_f'` per fold from statistics gathered in one pass over X.  Operands, outputs and the NaN
rule as for `kfold!`; a fold that carries nearly all of the state's information loses digits in the difference (Float32 first).
"""
function kfold_large!(km::Union{Nothing,DeviceArray{T}}, kv::Union{Nothing,DeviceArray{T}}, kl::Union{Nothing,DeviceArray{Float64}},
                      total::Union{Nothing,DeviceArray{Float64}}, info::DeviceArray{Int32}, X::DeviceArray{T}, y::DeviceArray{T},
                      s::DeviceArray{T}, mw::DeviceArray{T}, Tf::DeviceArray{T}; D::Int, N::Int, F::Int, B::Int, isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    nf = cld(N, F)
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : a.ptr
    dptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : a.ptr
    rc = if T === Float64
        ccall((:blr_kfold_large_batched_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, F, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, isotropic ? 0 : N, mw.ptr, D, Tf.ptr, D, D * D,
              ptr(km), N, ptr(kv), N, dptr(kl), nf, dptr(total), info.ptr)
    else
        ccall((:blr_kfold_large_batched_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, F, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, isotropic ? 0 : N, mw.ptr, D, Tf.ptr, D, D * D,
              ptr(km), N, ptr(kv), N, dptr(kl), nf, dptr(total), info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    loo_multi_batched!(lmean, lvar, llogpdf, total, info, X, Y, s, M, T; D, N, S, B, isotropic)

Exact leave-one-out predictives of the N observations with S targets each that B device-resident MULTI-OUTPUT states contain
(`blr_loo_multi_batched_*`): per observation n and column c the predictive of Y[n, c] given all the other data -- reference
`src/bayesian_linear_regression.jl:55-58` applied to each held-out point and column -- with the leverage of an input computed
once for its S columns; the states (M D×S×B, T D×D×B as `posterior_multi_batched!` / `update_multi_factor!` leave them) are not
modified.  X is D×N×B, Y N×S×B, s one variance (`isotropic`) or N×B.  lmean (N×S×B) and lvar (N×B: ONE per input) in the element
type, llogpdf (N×S×B) and total (S×B, Σ_n llogpdf in a fixed order) in Float64; any of the four may be `nothing`.  A leverage
within rounding of 1 gives NaN in lvar and in all S columns of that input (`get_stat("loo_degenerate")` counts it once);
info[b] > 0: a bad factor, else a bad variance, and that state's outputs are left untouched.
"""
function loo_multi_batched!(lm::Union{Nothing,DeviceArray{T}}, lv::Union{Nothing,DeviceArray{T}}, ll::Union{Nothing,DeviceArray{Float64}},
                            total::Union{Nothing,DeviceArray{Float64}}, info::DeviceArray{Int32}, X::DeviceArray{T}, Y::DeviceArray{T},
                            s::DeviceArray{T}, M::DeviceArray{T}, Tf::DeviceArray{T}; D::Int, N::Int, S::Int, B::Int,
                            isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : a.ptr
    dptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : a.ptr
    rc = if T === Float64
        ccall((:blr_loo_multi_batched_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Int64,
               Ptr{Cdouble}, Int64, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, S, X.ptr, D, D * N, Y.ptr, max(N, 1), N * S, nk, s.ptr, isotropic ? 0 : N, M.ptr, D, D * S,
              Tf.ptr, D, D * D, ptr(lm), max(N, 1), N * S, ptr(lv), N, dptr(ll), max(N, 1), N * S, dptr(total), S, info.ptr)
    else
        ccall((:blr_loo_multi_batched_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Int64,
               Ptr{Cdouble}, Int64, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, S, X.ptr, D, D * N, Y.ptr, max(N, 1), N * S, nk, s.ptr, isotropic ? 0 : N, M.ptr, D, D * S,
              Tf.ptr, D, D * D, ptr(lm), max(N, 1), N * S, ptr(lv), N, dptr(ll), max(N, 1), N * S, dptr(total), S, info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    kfold_multi_batched!(kmean, kvar, klogpdf, total, info, X, Y, s, M, T; D, N, S, F, B, isotropic)

Exact leave-fold-out (K-fold) predictives of the N observations with S targets each that B device-resident MULTI-OUTPUT states
contain (`blr_kfold_multi_batched_*`), for contiguous folds of F ≤ 64 observations and D ≤ 128: per column c what `kfold!` gives
on (M[:, c], Y[:, c]), with X read once and every fold's hat block factored once for its S columns; the states (M D×S×B, T D×D×B)
are not modified.  X is D×N×B, Y N×S×B, s one variance (`isotropic`) or N×B.  kmean (N×S×B) and kvar (N×B: ONE per input) in the
element type, klogpdf (nfolds×S×B, nfolds = cld(N, F): the JOINT log density of each fold and column) and total (S×B, Σ_f klogpdf
in a fixed order) in Float64; any of the four may be `nothing`.  A fold the state does not contain gives NaN in kvar of its
members and in all S columns (`get_stat("kfold_degenerate")` counts it once); info[b] > 0: a bad factor, else a bad variance, and
that state's outputs are left untouched.
"""
function kfold_multi_batched!(km::Union{Nothing,DeviceArray{T}}, kv::Union{Nothing,DeviceArray{T}}, kl::Union{Nothing,DeviceArray{Float64}},
                              total::Union{Nothing,DeviceArray{Float64}}, info::DeviceArray{Int32}, X::DeviceArray{T}, Y::DeviceArray{T},
                              s::DeviceArray{T}, M::DeviceArray{T}, Tf::DeviceArray{T}; D::Int, N::Int, S::Int, F::Int, B::Int,
                              isotropic::Bool) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    nf = max(cld(N, F), 1)
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : a.ptr
    dptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : a.ptr
    rc = if T === Float64
        ccall((:blr_kfold_multi_batched_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Int64,
               Ptr{Cdouble}, Int64, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, S, F, X.ptr, D, D * N, Y.ptr, max(N, 1), N * S, nk, s.ptr, isotropic ? 0 : N, M.ptr, D, D * S,
              Tf.ptr, D, D * D, ptr(km), max(N, 1), N * S, ptr(kv), N, dptr(kl), nf, nf * S, dptr(total), S, info.ptr)
    else
        ccall((:blr_kfold_multi_batched_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Int64,
               Ptr{Cdouble}, Int64, Ptr{Int32}),
              h, MEM_DEVICE, COLVECS, B, D, N, S, F, X.ptr, D, D * N, Y.ptr, max(N, 1), N * S, nk, s.ptr, isotropic ? 0 : N, M.ptr, D, D * S,
              Tf.ptr, D, D * D, ptr(km), max(N, 1), N * S, ptr(kv), N, dptr(kl), nf, nf * S, dptr(total), S, info.ptr)
    end
    check(h, rc)
    return nothing
end

"""
    loo(fx, y) -> (mean, var, logpdf)

Leave-one-out predictives of the observations y at fx.x: the posterior of `fused` (reference `:60-69`), then one
`blr_loo_batched_*` call on it (host memspace) -- what a loop of `forget` / `condition` per observation gives.  var includes
the noise, as `var(fx)` does; logpdf is Float64 (`sum(logpdf)` is the LOO-CV score).  Dense noise is not offloaded.
"""
function loo(fx::FiniteGP, y::AbstractVector{<:Real})
    fb = to_blr(fx)
    xl, nz = xlayout(fb.x), noise(fb.Σy)
    (xl === nothing || nz === nothing || nz[2] == DENSEN) && throw(ArgumentError("loo: ColVecs / RowVecs inputs and isotropic or Diagonal noise"))
    X, layout, ldx, D, N = xl
    T = eltype(X)
    r = fused(fb, y, true)
    r === nothing && throw(ArgumentError("loo: the prior is not offloadable"))
    _, mw′, Tp, _ = r
    yv = convert(Vector{T}, y)
    s, nk, _ = nz
    lm, lv, ll = Vector{T}(undef, N), Vector{T}(undef, N), Vector{Float64}(undef, N)
    total = Ref{Cdouble}(0.0); info = Ref{Int32}(0)
    h = handle()
    rc = GC.@preserve X yv s mw′ Tp lm lv ll begin
        if T === Float64
            ccall((:blr_loo_batched_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ref{Cdouble}, Ref{Int32}),
                  h, MEM_HOST, layout, 1, D, N, X, ldx, 0, yv, 0, nk, s, 0, mw′, 0, Tp, D, 0, lm, N, lv, N, ll, N, total, info)
        else
            ccall((:blr_loo_batched_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ref{Cdouble}, Ref{Int32}),
                  h, MEM_HOST, layout, 1, D, N, X, ldx, 0, yv, 0, nk, s, 0, mw′, 0, Tp, D, 0, lm, N, lv, N, ll, N, total, info)
        end
    end
    check(h, rc)
    check(h, info[])
    return lm, lv, ll
end

"""
    logpdf_grid!(lp, best, mw_best, T_best, info, X, y, s, mw, Lw, alpha, tau; D, N, B, G, isotropic, diagonal_prior,
                 noise_stride = isotropic ? 1 : N)

Evidence of each of B device-resident data sets under G settings Λw = alpha[g] Lw, Σy = tau[g] s (one grid shared by all data
sets) from ONE pass over X (`blr_logpdf_grid_*`; reference `src/bayesian_linear_regression.jl:55-58` per setting): lp is G×B
(Float64), info G×B, best (Int64, 0-based setting of the largest finite evidence, -1 if none) B or `nothing`, mw_best D×B and
T_best D×D×B the posterior at that setting or `nothing`.  Lw is D×B (`diagonal_prior`) or D×D×B.  s holds one variance per data
set (`isotropic`, length B) or N×B; `noise_stride = 0` makes all data sets share the first one (or the first N).
"""
function logpdf_grid!(lp::DeviceArray{Float64}, best::Union{Nothing,DeviceArray{Int64}}, mw_best::Union{Nothing,DeviceArray{T}},
                      T_best::Union{Nothing,DeviceArray{T}}, info::DeviceArray{Int32}, X::DeviceArray{T}, y::DeviceArray{T},
                      s::DeviceArray{T}, mw::DeviceArray{T}, Lw::DeviceArray{T}, alpha::DeviceArray{T}, tau::DeviceArray{T};
                      D::Int, N::Int, B::Int, G::Int, isotropic::Bool, diagonal_prior::Bool,
                      noise_stride::Int = isotropic ? 1 : N) where {T<:Elt}
    h = handle()
    nk = isotropic ? ISOTROPIC : DIAGONALN
    pk = diagonal_prior ? P_DIAG : P_DENSE
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : a.ptr
    iptr(a) = a === nothing ? Ptr{Int64}(C_NULL) : a.ptr
    rc = if T === Float64
        ccall((:blr_logpdf_grid_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Int64,
               Int64, Ptr{Int32}, Int64),
              h, MEM_DEVICE, COLVECS, B, D, N, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, noise_stride, pk, mw.ptr, D, Lw.ptr, D,
              diagonal_prior ? D : D * D, G, alpha.ptr, 0, tau.ptr, 0, lp.ptr, G, iptr(best), ptr(mw_best), D, ptr(T_best), D, D * D,
              info.ptr, G)
    else
        ccall((:blr_logpdf_grid_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Int64,
               Int64, Ptr{Int32}, Int64),
              h, MEM_DEVICE, COLVECS, B, D, N, X.ptr, D, D * N, y.ptr, N, nk, s.ptr, noise_stride, pk, mw.ptr, D, Lw.ptr, D,
              diagonal_prior ? D : D * D, G, alpha.ptr, 0, tau.ptr, 0, lp.ptr, G, iptr(best), ptr(mw_best), D, ptr(T_best), D, D * D,
              info.ptr, G)
    end
    check(h, rc)
    return nothing
end

"""
    logpdf_grid_ragged!(lp, best, mw_best, T_best, info, X, offsets, y, s, mw, Lw, alpha, tau; D, G, isotropic, diagonal_prior)

`logpdf_grid!` for B = length(offsets) - 1 data sets with UNEQUAL observation counts in one call (`blr_logpdf_grid_ragged_*`;
reference `src/bayesian_linear_regression.jl:55-58` per setting under a map over fxs of different lengths), everything device
resident except `offsets` (a host `Vector{Int64}`, zero based, B + 1 non-decreasing entries): data set b owns the columns
offsets[b]+1:offsets[b+1] of X (D×offsets[end], ColVecs) and the same entries of y; s holds B variances (`isotropic`) or
offsets[end]; mw is D×B, Lw D×B (`diagonal_prior`) or D×D×B; one grid alpha, tau (length G) shared by all; outputs as
`logpdf_grid!`.  Every output of data set b has the bits of `logpdf_grid!` with B = 1 on its slice.
"""
function logpdf_grid_ragged!(lp::DeviceArray{Float64}, best::Union{Nothing,DeviceArray{Int64}}, mw_best::Union{Nothing,DeviceArray{T}},
                             T_best::Union{Nothing,DeviceArray{T}}, info::DeviceArray{Int32}, X::DeviceArray{T}, offsets::Vector{Int64},
                             y::DeviceArray{T}, s::DeviceArray{T}, mw::DeviceArray{T}, Lw::DeviceArray{T}, alpha::DeviceArray{T},
                             tau::DeviceArray{T}; D::Int, G::Int, isotropic::Bool, diagonal_prior::Bool) where {T<:Elt}
    h = handle()
    B = length(offsets) - 1
    nk = isotropic ? ISOTROPIC : DIAGONALN
    pk = diagonal_prior ? P_DIAG : P_DENSE
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : a.ptr
    iptr(a) = a === nothing ? Ptr{Int64}(C_NULL) : a.ptr
    rc = GC.@preserve offsets begin
        if T === Float64
            ccall((:blr_logpdf_grid_ragged_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Int64,
                   Int64, Ptr{Int32}, Int64),
                  h, MEM_DEVICE, COLVECS, B, D, offsets, X.ptr, D, y.ptr, nk, s.ptr, isotropic ? 1 : 0, pk, mw.ptr, D, Lw.ptr, D,
                  diagonal_prior ? D : D * D, G, alpha.ptr, 0, tau.ptr, 0, lp.ptr, G, iptr(best), ptr(mw_best), D, ptr(T_best), D, D * D,
                  info.ptr, G)
        else
            ccall((:blr_logpdf_grid_ragged_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
                   Ptr{T}, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Int64,
                   Int64, Ptr{Int32}, Int64),
                  h, MEM_DEVICE, COLVECS, B, D, offsets, X.ptr, D, y.ptr, nk, s.ptr, isotropic ? 1 : 0, pk, mw.ptr, D, Lw.ptr, D,
                  diagonal_prior ? D : D * D, G, alpha.ptr, 0, tau.ptr, 0, lp.ptr, G, iptr(best), ptr(mw_best), D, ptr(T_best), D, D * D,
                  info.ptr, G)
        end
    end
    check(h, rc)
    return nothing
end

"""
    logpdf_grid(fx, y, prior_scales, noise_scales) -> (logpdf, best, mw_best, T_best)

Evidence of (fx, y) under every (prior scale, noise scale) pair -- logpdf[j, i] for noise_scales[j], prior_scales[i] -- the
1-based (j, i) of the largest finite one, and the posterior mean and factor at that setting, in one library call (host
memspace).  Isotropic or Diagonal noise; a Diagonal or dense prior precision (a PDMat prior is passed as U'U).
"""
function logpdf_grid(fx::FiniteGP, y::AbstractVector{<:Real}, prior_scales::AbstractVector{<:Real}, noise_scales::AbstractVector{<:Real})
    fb = to_blr(fx)
    xl, nz = xlayout(fb.x), noise(fb.Σy)
    Λ = fb.f.Λw isa AbstractPDMat ? Symmetric(Matrix(fb.f.Λw)) : fb.f.Λw   # U'U, a small D x D product on the host
    pr = prior(Λ)
    (xl === nothing || nz === nothing || pr === nothing || nz[2] == DENSEN) &&
        throw(ArgumentError("logpdf_grid: ColVecs / RowVecs inputs, isotropic or Diagonal noise, Diagonal or dense prior"))
    X, layout, ldx, D, N = xl
    T = eltype(X)
    yv, mw = convert(Vector{T}, y), convert(Vector{T}, fb.f.mw)
    s, nk, _ = nz
    Lw, pk, ldl = pr
    na, nt = length(prior_scales), length(noise_scales)
    G = na * nt
    G == 0 && throw(ArgumentError("logpdf_grid: prior_scales and noise_scales must not be empty"))
    a = T[prior_scales[i] for i in 1:na for _ in 1:nt]   # prior scale slowest
    t = T[noise_scales[j] for _ in 1:na for j in 1:nt]
    lp = Vector{Float64}(undef, G); info = zeros(Int32, G); best = Int64[-1]
    mw′ = Vector{T}(undef, D); Tp = Matrix{T}(undef, D, D)
    h = handle()
    rc = GC.@preserve X yv s mw Lw a t lp info best mw′ Tp begin
        if T === Float64
            ccall((:blr_logpdf_grid_f64, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Int64,
               Int64, Ptr{Int32}, Int64),
                  h, MEM_HOST, layout, 1, D, N, X, ldx, 0, yv, 0, nk, s, 0, pk, mw, 0, Lw, ldl, 0, G, a, 0, t, 0, lp, G, best, mw′, 0, Tp, D, 0,
                  info, G)
        else
            ccall((:blr_logpdf_grid_f32, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64,
               Ptr{T}, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{T}, Int64, Ptr{T}, Int64,
               Int64, Ptr{Int32}, Int64),
                  h, MEM_HOST, layout, 1, D, N, X, ldx, 0, yv, 0, nk, s, 0, pk, mw, 0, Lw, ldl, 0, G, a, 0, t, 0, lp, G, best, mw′, 0, Tp, D, 0,
                  info, G)
        end
    end
    check(h, rc)
    best[1] < 0 && check(h, info[1])
    k = Int(best[1])
    return reshape(lp, nt, na), (k % nt + 1, k ÷ nt + 1), mw′, Tp
end

"""
    rand_batched!(Y, W, info, X, mw, Tf, Z1, Z2; D, N, S, B, shared_x=false, s=nothing)

Draws from B device-resident states, the step that closes a Thompson-sampling loop around `update_factor!` on `DeviceArray`s:
W_b = mw_b + T_b \ Z1_b (D×S) and Y_b = X_b' W_b (N×S), plus sqrt.(s) .* Z2_b when `s` (one variance, a `DeviceArray` of
length 1) is given.  mw is D×B and Tf D×D×B exactly as `posterior_batched!` / `update_factor!` keep them; X is D×N×B, or one
D×N candidate set for the whole batch (`shared_x`); Z1 D×S×B and Z2 N×S×B hold the normals (drawn on the host, reference
:51-52).  `Y`, `W` or `Z2` may be `nothing`.  info[b] > 0: that state's factor has a non-positive diagonal entry; its outputs
are left untouched.  Reference semantics per regressor: `:49-53`, `sampling_functions.jl:16-49`.
"""
function rand_batched!(Y::Union{Nothing,DeviceArray{T}}, W::Union{Nothing,DeviceArray{T}}, info::DeviceArray{Int32}, X::DeviceArray{T},
                       mw::DeviceArray{T}, Tf::DeviceArray{T}, Z1::DeviceArray{T}, Z2::Union{Nothing,DeviceArray{T}};
                       D::Int, N::Int, S::Int, B::Int, shared_x::Bool=false, s::Union{Nothing,DeviceArray{T}}=nothing) where {T<:Elt}
    h = handle()
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : a.ptr
    noisy = Z2 !== nothing && s !== nothing
    rc = rand_batched_call(h, MEM_DEVICE, COLVECS, B, D, N, S, X.ptr, D, shared_x ? 0 : D * N, ISOTROPIC, noisy ? s.ptr : Ptr{T}(C_NULL),
                           0, P_UPPER, mw.ptr, D, Tf.ptr, D, D * D, Z1.ptr, D, D * S, noisy ? Z2.ptr : Ptr{T}(C_NULL), N, N * S,
                           ptr(W), D, D * S, ptr(Y), N, N * S, info.ptr, T)
    check(h, rc)
    return nothing
end

# blr_rand_multi_batched_* (include/blr_mi355x.h): R draws from each of the S column posteriors (M: D x S per regressor, one shared
# factor) of B regressors, draw j = c R + r
function rand_multi_batched_call(h, memspace, layout, B, D, N, S, R, X, ldx, strideX, nk, s, strides, pk, M, ldm, strideM, Lw, ldl, strideLw,
                                 Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y, ldy, strideY, info, ::Type{T}) where {T<:Elt}
    if T === Float64
        ccall((:blr_rand_multi_batched_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Int32}),
              h, memspace, layout, B, D, N, S, R, X, ldx, strideX, nk, s, strides, pk, M, ldm, strideM, Lw, ldl, strideLw,
              Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y, ldy, strideY, info)
    else
        ccall((:blr_rand_multi_batched_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Int64, Int64, Int64, Ptr{T}, Int64, Int64, Cint, Ptr{T}, Int64, Cint, Ptr{T}, Int64, Int64,
               Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{T}, Int64, Int64, Ptr{Int32}),
              h, memspace, layout, B, D, N, S, R, X, ldx, strideX, nk, s, strides, pk, M, ldm, strideM, Lw, ldl, strideLw,
              Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y, ldy, strideY, info)
    end
end

"""
    rand_multi_batched!(Y, W, info, X, M, Tf, Z1, Z2; D, N, S, R, B, shared_x=false, s=nothing)

R draws from each of the S column posteriors of B device-resident multi-output states (M D×S×B and Tf D×D×B exactly as
`posterior_multi_batched!` / `update_multi_factor!` keep them), draw j = (c-1)R + r: W_b[:, j] = M_b[:, c] + T_b \\ Z1_b[:, j]
(D×S·R) and Y_b = X_b' W_b (N×S·R), plus sqrt.(s) .* Z2_b when `s` (one variance, a `DeviceArray` of length 1) is given.  X is
D×N×B, or one D×N candidate set for the whole batch (`shared_x`); Z1 D×S·R×B and Z2 N×S·R×B hold the normals (drawn on the host
column by column, reference :51-52).  `Y`, `W` or `Z2` may be `nothing`.  info[b] > 0: that state's factor has a non-positive
diagonal entry; its outputs are left untouched.  Reference semantics per column: `:49-53`, `sampling_functions.jl:16-49`.
"""
function rand_multi_batched!(Y::Union{Nothing,DeviceArray{T}}, W::Union{Nothing,DeviceArray{T}}, info::DeviceArray{Int32}, X::DeviceArray{T},
                             M::DeviceArray{T}, Tf::DeviceArray{T}, Z1::DeviceArray{T}, Z2::Union{Nothing,DeviceArray{T}};
                             D::Int, N::Int, S::Int, R::Int, B::Int, shared_x::Bool=false,
                             s::Union{Nothing,DeviceArray{T}}=nothing) where {T<:Elt}
    h = handle()
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : a.ptr
    noisy = Z2 !== nothing && s !== nothing
    rc = rand_multi_batched_call(h, MEM_DEVICE, COLVECS, B, D, N, S, R, X.ptr, D, shared_x ? 0 : D * N, ISOTROPIC,
                                 noisy ? s.ptr : Ptr{T}(C_NULL), 0, P_UPPER, M.ptr, D, D * S, Tf.ptr, D, D * D, Z1.ptr, D, D * S * R,
                                 noisy ? Z2.ptr : Ptr{T}(C_NULL), N, N * S * R, ptr(W), D, D * S * R, ptr(Y), N, N * S * R, info.ptr, T)
    check(h, rc)
    return nothing
end

# ---- one Julia process per GPU: the path's single exchange through RCCL, called directly (SURVEY.md 8e) ------------------
"rank 0: 128 opaque bytes to ship to the other ranks (Distributed.jl, a file, MPI ...)"
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    rc = GC.@preserve id ccall((:blr_comm_unique_id, LIB), Cint, (Ptr{Cvoid},), id)
    rc == 0 || error("blr_comm_unique_id failed with code $rc (librccl missing?)")
    id
end
function comm_init!(nranks::Integer, rank::Integer, id::Vector{UInt8})
    h = handle()
    GC.@preserve id check(h, ccall((:blr_comm_init, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}), h, nranks, rank, id))
end
comm_destroy!() = (h = handle(); check(h, ccall((:blr_comm_destroy, LIB), Cint, (Ptr{Cvoid},), h)))

"""
    posterior_nsharded!(mw_post, T_post, logpdf, info, stats, scal, X, y, s, mw, Λdiag; D, N_local, N_total)

ONE regressor whose observations are split over the ranks of `comm_init!` (SURVEY §8e): this rank's `N_local` columns of X
(D×N_local, device), diagonal noise `s`, diagonal prior `Λdiag`; `stats` ((128⌈D/128⌉+128) × 128⌈D/128⌉) and `scal` (2 Float64)
are device scratch.  Every rank ends with the same posterior (`mw_post`, upper factor `T_post`) and evidence of all `N_total`
observations: local statistics, one in-place all-reduce, redundant D×D finish.
"""
function posterior_nsharded!(mw_post::DeviceArray{T}, T_post::DeviceArray{T}, lp::DeviceArray{Float64}, info::DeviceArray{Int32},
                             stats::DeviceArray{T}, scal::DeviceArray{Float64}, X::DeviceArray{T}, y::DeviceArray{T},
                             s::DeviceArray{T}, mw::DeviceArray{T}, Λdiag::DeviceArray{T}; D::Int, N_local::Int, N_total::Int) where {T<:Elt}
    h = handle()
    lds = 128 * cld(D, 128) + 128
    rc = if T === Float64
        ccall((:blr_posterior_nsharded_f64, LIB), Cint,
              (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Cint, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{Cdouble}, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, COLVECS, D, N_local, N_total, X.ptr, D, y.ptr, DIAGONALN, s.ptr, P_DIAG, mw.ptr, Λdiag.ptr, 1, stats.ptr, lds,
              scal.ptr, mw_post.ptr, T_post.ptr, D, Ptr{T}(C_NULL), D, lp.ptr, info.ptr)
    else
        ccall((:blr_posterior_nsharded_f32, LIB), Cint,
              (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{T}, Int64, Ptr{T}, Cint, Ptr{T}, Cint, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64,
               Ptr{Cdouble}, Ptr{T}, Ptr{T}, Int64, Ptr{T}, Int64, Ptr{Cdouble}, Ptr{Int32}),
              h, COLVECS, D, N_local, N_total, X.ptr, D, y.ptr, DIAGONALN, s.ptr, P_DIAG, mw.ptr, Λdiag.ptr, 1, stats.ptr, lds,
              scal.ptr, mw_post.ptr, T_post.ptr, D, Ptr{T}(C_NULL), D, lp.ptr, info.ptr)
    end
    check(h, rc)
    return nothing
end

comm_size() = ccall((:blr_comm_size, LIB), Cint, (Ptr{Cvoid},), handle())
comm_rank() = ccall((:blr_comm_rank, LIB), Cint, (Ptr{Cvoid},), handle())
"all-gather of every rank's `count` log evidences + the same fixed-order sum on every rank; returns the total"
function logpdf_allgather_sum!(lp_all::DeviceArray{Float64}, lp_local::DeviceArray{Float64}, count::Integer)
    tot = DeviceArray{Float64}(1)
    h = handle()
    check(h, ccall((:blr_logpdf_allgather_sum, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                   h, count, lp_local.ptr, lp_all.ptr, tot.ptr))
    download!(Vector{Float64}(undef, 1), tot)[1]
end
"in-place sum over ranks of a device buffer (the `stats` exchange of the N-sharded single regressor)"
function allreduce_sum!(buf::DeviceArray{T}) where {T<:Elt}
    h = handle()
    check(h, ccall((:blr_allreduce_sum, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64), h, T === Float64 ? 1 : 0, buf.ptr, buf.len))
    buf
end

# ---- drop-in: replace the reference's methods for the session ------------------------------------------------------------
"""
    install_overrides!()

Redefine `AbstractGPs.logpdf / posterior / mean / var / cov / mean_and_var / mean_and_cov / rand` on
`FiniteGP{<:BayesianLinearRegressor}` and `FiniteGP{<:BasisFunctionRegressor}` (reference
src/bayesian_linear_regression.jl:33-69, src/basis_function_regression.jl:46-65) and the `Random` hooks of
src/sampling_functions.jl:23-49 so that unmodified user code runs on the MI355X path.  Method overwriting is deliberate and
explicit (Julia prints one warning per method); inputs the device path does not take still reach the reference's code.
"""
function install_overrides!()
    # the EXACT signatures of the reference (one per regressor type), so these definitions replace its methods
    for R in (:BayesianLinearRegressor, :BasisFunctionRegressor)
        @eval begin
            AbstractGPs.logpdf(fx::FiniteGP{<:$R}, y::AbstractVector{<:Real}) = BLRMI355X.logpdf(fx, y)
            AbstractGPs.logpdf(fx::FiniteGP{<:$R}, Y::AbstractMatrix{<:Real}) = BLRMI355X.logpdf(fx, Y)
            AbstractGPs.posterior(fx::FiniteGP{<:$R}, y::AbstractVector{<:Real}) = BLRMI355X.posterior(fx, y)
            AbstractGPs.mean(fx::FiniteGP{<:$R}) = BLRMI355X.mean(fx)
            AbstractGPs.var(fx::FiniteGP{<:$R}) = BLRMI355X.var(fx)
            AbstractGPs.cov(fx::FiniteGP{<:$R}) = BLRMI355X.cov(fx)
            AbstractGPs.mean_and_var(fx::FiniteGP{<:$R}) = BLRMI355X.mean_and_var(fx)
            AbstractGPs.mean_and_cov(fx::FiniteGP{<:$R}) = BLRMI355X.mean_and_cov(fx)
            AbstractGPs.rand(rng::AbstractRNG, fx::FiniteGP{<:$R}, S::Int) = BLRMI355X.rand(rng, fx, S)
        end
    end
    @eval begin
        # the reference's Sampler hook returns the regressor ITSELF (sampling_functions.jl:23-25), so `rand(rng, f)` dispatches
        # on the regressor type (:27), not on a SamplerTrivial
        Random.rand(rng::AbstractRNG, b::BLRLike) = BLRMI355X.rand(rng, b)
        Random.rand(rng::AbstractRNG, b::BLRLike, dims::Dims) = BLRMI355X.rand(rng, b, dims)
        Random.rand!(rng::AbstractRNG, A::AbstractArray{<:BLRFunctionSample}, b::BLRLike) = BLRMI355X.rand!(rng, A, b)
    end
    return nothing
end

end # module
