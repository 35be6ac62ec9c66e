// utilities.hpp -- CLI, timer-tree printing and COO->CRS conversion
// (reference utilities/utilities.hpp:12-108, :154-324, :326-367).  Same flags
// and the same output layout.  Extra, MI355X-specific: the <matrix> argument
// may be a generator string instead of a file (the reference does the same
// with SCAMAC strings when built with -DUSE_SCAMAC, main.cpp:48-54):
//     hpcg:N | hpcg:NX,NY,NZ | anderson:L[,shift=S][,W=w][,t=t][,seed=k] | fem:NX[,NY,NZ][,keep=K][,seed=k] | unstr:NX[,NY,NZ][,keep=K][,seed=k]
// and `-unfused` / `-dev K` select the kernel-by-kernel CG and the device;
// `-perm mc` applies the multi-colour reordering of utilities/permute.hpp; `-p ilu0it` is ILU(0) with iterative
// triangular solves (bis_itrsv) and `-inner K` their step count (also the inner sweeps of 2st / s2st); `-p fsai` is the
// factorized sparse approximate inverse of bis_mat_fsai, applied as two SpMVs; `-pprec 32` rounds the factors those two
// types apply by SpMV to fp32 (bis_mat_round_f32); `-p mg` is one V-cycle of the aggregation multigrid hierarchy of bis_mg_create
// (or, with `-mg cycle=w|k|kgcr`, one W- or K-cycle) and `-mg key=value,...` sets its parameters; the method `-fgm` is flexible
// GMRES(m) on the device schedule bis_fgmres_* (methods/fgmres.hpp), which takes every -p type, the K-cycles included; the method
// `-mr` is MINRES for symmetric, possibly indefinite matrices on the device schedule bis_minres_* (methods/minres.hpp);
// the method `-idr` is IDR(s) for nonsymmetric matrices on the device schedule bis_idr_* (methods/idr.hpp) and `-ids S` its s (default 4);
// `-p bj` is block Jacobi (bis_bj_create) on blocks of `-bs N` consecutive rows (default: the dof of the grid hint);
// the method `-lsmr` is LSMR for least-squares problems on the device schedule bis_lsmr_* (methods/lsmr.hpp), the one method that
// takes a rectangular .mtx; `-damp L` is its Tikhonov parameter and `-colscale` scales the columns of A to norm 1;
// the method `-eig K` is the thick-restart Lanczos eigensolver on the device schedule bis_eigs_* (methods/eigs.hpp): the K smallest
// (`-which sa`, the default), largest (`la`) or largest in magnitude (`lm`) eigenpairs of a symmetric matrix with a basis of `-ncv M`;
// the method `-svd K` is thick-restart Lanczos bidiagonalisation on the device schedule bis_svds_* (methods/svds.hpp): the K largest
// (`-which lm`, the default) or smallest (`sm`) singular triplets of a matrix of any shape (a rectangular .mtx is read as for -lsmr).
#pragma once

#include <sys/stat.h>

#include "../common.hpp"
#include "../sparse_matrix.hpp"

inline void parse_cli(Args *a, int argc, char *argv[]) {
    if (argc < 3) {
        printf("ERROR: parse_cli: Not enough arguments given. A call should contain:"
               "\n%s <matrix> <method> [extra_features]\n", argv[0]);
        exit(EXIT_FAILURE);
    }
    a->matrix_file_name = argv[1];
    const std::string st = argv[2];
    if (st == "-j") a->method = SolverType::Jacobi;
    else if (st == "-gs") a->method = SolverType::GaussSeidel;
    else if (st == "-sgs") a->method = SolverType::SymmetricGaussSeidel;
    else if (st == "-cg") a->method = SolverType::ConjugateGradient;
    else if (st == "-gm") a->method = SolverType::GMRES;
    else if (st == "-bi") a->method = SolverType::BiCGSTAB;
    else if (st == "-fgm") a->method = SolverType::FGMRES;
    else if (st == "-mr") a->method = SolverType::MINRES;
    else if (st == "-idr") a->method = SolverType::IDR;
    else if (st == "-lsmr") a->method = SolverType::LSMR;
    else if (st == "-eig") {
        a->method = SolverType::Eigs;
        char *end = nullptr;
        const long kk = argc > 3 ? strtol(argv[3], &end, 10) : 0;
        if (argc <= 3 || end == argv[3] || *end != '\0' || kk < 1 || kk > 63) {
            fprintf(stderr, "ERROR: -eig K: the number of wanted eigenpairs, 1 <= K <= 63\n");
            exit(EXIT_FAILURE);
        }
        eigs_k() = (int)kk;
    }
    else if (st == "-svd") {
        a->method = SolverType::SVDS;
        char *end = nullptr;
        const long kk = argc > 3 ? strtol(argv[3], &end, 10) : 0;
        if (argc <= 3 || end == argv[3] || *end != '\0' || kk < 1 || kk > 63) {
            fprintf(stderr, "ERROR: -svd K: the number of wanted singular triplets, 1 <= K <= 63\n");
            exit(EXIT_FAILURE);
        }
        svds_k() = (int)kk;
    }
    else {
        printf("ERROR: parse_cli: Please choose an available solver:"
               "\n-j (Jacobi)\n-gs (Gauss-Seidel)\n-sgs (Symmetric Gauss-Seidel)"
               "\n-gm ([Preconditioned] GMRES)\n-cg ([Preconditioned] Conjugate Gradient)"
               "\n-bi ([Preconditioned] BiCGSTAB)"
               "\n-fgm ([Preconditioned] flexible GMRES, right-preconditioned)"
               "\n-mr ([Preconditioned] MINRES, symmetric indefinite matrices)"
               "\n-idr ([Preconditioned] IDR(s), nonsymmetric matrices, -ids S = 1..8)"
               "\n-lsmr (LSMR, least-squares problems with rectangular matrices, -damp L >= 0, -colscale)"
               "\n-eig K (thick-restart Lanczos, the K extreme eigenpairs of a symmetric matrix, -which sa|la|lm, -ncv M)"
               "\n-svd K (thick-restart Lanczos bidiagonalisation, the K largest or smallest singular triplets of a matrix of any shape, -which lm|sm, -ncv M)\n");
        exit(EXIT_FAILURE);
    }
    for (int i = a->method == SolverType::Eigs || a->method == SolverType::SVDS ? 4 : 3; i < argc; ++i) { // (-eig K, -svd K: argv[3] is K)
        const std::string arg = argv[i];
        if (arg == "-p") {
            if (i + 1 >= argc) {
                printf("ERROR: parse_cli: Not enough arguments given. Some extra features need "
                       "additional arguments. Example:\n%s <matrix> <method> -p gs\n", argv[0]);
                exit(EXIT_FAILURE);
            }
            const std::string pt = argv[++i];
            static const std::map<std::string, PrecondType> pcs = {
                {"j", PrecondType::Jacobi}, {"gs", PrecondType::GaussSeidel},
                {"bgs", PrecondType::BackwardsGaussSeidel}, {"sgs", PrecondType::SymmetricGaussSeidel},
                {"2st", PrecondType::TwoStageGS}, {"s2st", PrecondType::SymmetricTwoStageGS},
                {"ilu0", PrecondType::ILU0}, {"ilu0it", PrecondType::ILU0Iter},
                {"fsai", PrecondType::FSAI}, {"mg", PrecondType::MG}, {"bj", PrecondType::BlockJacobi}};
            auto it = pcs.find(pt);
            if (it == pcs.end()) {
                fprintf(stderr, "ERROR: assign_cli_inputs: Please choose an available preconditioner type: "
                                "\n-p j (Jacobi)\n-p gs (Gauss-Seidel)\n-p bgs (Backwards Gauss-Seidel)"
                                "\n-p sgs (Symmetric Gauss-Seidel)\n-p 2st (2 Stage Gauss-Seidel)"
                                "\n-p s2st (Symmetric 2 Stage Gauss-Seidel)\n-p ilu0 (Incomplete LU with 0 fill-in)"
                                "\n-p ilu0it (Incomplete LU with 0 fill-in, -inner K Jacobi-Richardson steps per triangular solve)"
                                "\n-p fsai (Factorized sparse approximate inverse on the pattern of tril(A))"
                                "\n-p mg (Aggregation multigrid cycle, -mg nu=1,cs=4,limit=256,levels=10,scale=1,omega=0,coarsening=auto|grid|mis,cycle=v|w|k|kgcr,klev=0,smooth=0|1,pomega=X,smoother=jacobi|cheb,degree=2,ratio=4,est=10,safety=1.1)"
                                "\n-p bj (Block Jacobi on blocks of -bs N consecutive rows, N = 1..32; default: the dof of the grid hint)\n");
                exit(EXIT_FAILURE);
            }
            a->preconditioner = it->second;
            a->precond_given = true;
        } else if (arg == "-scale" && i + 1 < argc) { a->num_scale = (bool)atoi(argv[++i]); a->scale_given = true; }
        else if (arg == "-rl" && i + 1 < argc) a->restart_length = atoi(argv[++i]);
        else if (arg == "-inner" && i + 1 < argc) {
            a->inner_iters = atoi(argv[++i]);
            if (a->inner_iters < 0) {
                fprintf(stderr, "ERROR: -inner K: K >= 0\n");
                exit(EXIT_FAILURE);
            }
            precond_inner_iters() = a->inner_iters;
        }
        else if (arg == "-pprec" && i + 1 < argc) {
            a->pprec = atoi(argv[++i]);
            if (a->pprec != 32 && a->pprec != 64) {
                fprintf(stderr, "ERROR: -pprec 32|64\n");
                exit(EXIT_FAILURE);
            }
            precond_value_bits() = a->pprec;
        }
        else if (arg == "-bs" && i + 1 < argc) {
            const std::string v = argv[++i];
            const int bs = v.find_first_not_of("0123456789") == std::string::npos && v.size() <= 3 ? atoi(v.c_str()) : 0;
            if (bs < 1 || bs > 32) {
                fprintf(stderr, "ERROR: -bs N: the rows per block of -p bj, 1 <= N <= 32\n");
                exit(EXIT_FAILURE);
            }
            precond_block_size() = bs;
        }
        else if (arg == "-fill" && i + 1 < argc) {
            const std::string v = argv[++i];
            const int k = v.find_first_not_of("0123456789") == std::string::npos && v.size() <= 2 ? atoi(v.c_str()) : -1;
            if (k < 0 || k > 16) {
                fprintf(stderr, "ERROR: -fill K: the level-of-fill of -p ilu0 / -p ilu0it, 0 <= K <= 16\n");
                exit(EXIT_FAILURE);
            }
            a->fill_level = k;
            a->fill_given = true;
            precond_fill_level() = k;
        }
        else if (arg == "-ids" && i + 1 < argc) {
            const std::string v = argv[++i];
            const int sd = v.find_first_not_of("0123456789") == std::string::npos && !v.empty() && v.size() <= 2 ? atoi(v.c_str()) : 0;
            if (sd < 1 || sd > 8) {
                fprintf(stderr, "ERROR: -ids S: the dimension of the shadow space of -idr, 1 <= S <= 8\n");
                exit(EXIT_FAILURE);
            }
            a->ids_given = true;
            idr_shadow_dim() = sd;
        }
        else if (arg == "-damp" && i + 1 < argc) {
            char *end = nullptr;
            a->damp = strtod(argv[++i], &end);
            if (end == argv[i] || *end != '\0' || !(a->damp >= 0.0) || !std::isfinite(a->damp)) {
                fprintf(stderr, "ERROR: -damp L: the Tikhonov parameter of -lsmr, L >= 0 and finite\n");
                exit(EXIT_FAILURE);
            }
            a->damp_given = true;
        }
        else if (arg == "-colscale") a->colscale = true;
        else if (arg == "-which" && i + 1 < argc) {
            const std::string w = argv[++i];
            if (a->method == SolverType::SVDS) {
                if (w != "lm" && w != "sm") {
                    fprintf(stderr, "ERROR: -which lm|sm: the end of the spectrum -svd K looks for (largest, smallest)\n");
                    exit(EXIT_FAILURE);
                }
                svds_which() = w == "lm" ? BIS_SVDS_LM : BIS_SVDS_SM;
            } else if (w != "sa" && w != "la" && w != "lm") {
                fprintf(stderr, "ERROR: -which sa|la|lm: the end of the spectrum -eig K looks for (smallest, largest, largest in magnitude)\n");
                exit(EXIT_FAILURE);
            }
            if (a->method != SolverType::SVDS) eigs_which() = w == "sa" ? BIS_EIGS_SA : w == "la" ? BIS_EIGS_LA : BIS_EIGS_LM;
            a->which_given = true;
        }
        else if (arg == "-ncv" && i + 1 < argc) {
            char *end = nullptr;
            const long m = strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end != '\0' || m < 2 || m > 64) {
                if (a->method == SolverType::SVDS) fprintf(stderr, "ERROR: -ncv M: the basis size of -svd K, K < M <= min(rows, cols, 64)\n");
                else fprintf(stderr, "ERROR: -ncv M: the basis size of -eig K, K < M <= min(n, 64)\n");
                exit(EXIT_FAILURE);
            }
            (a->method == SolverType::SVDS ? svds_ncv() : eigs_ncv()) = (int)m;
            a->ncv_given = true;
        }
        else if (arg == "-mg" && i + 1 < argc) {
            bis_mg_params &p = precond_mg_params();
            std::stringstream ss(argv[++i]);
            std::string item, pomega_item, cheb_item;
            const char *mg_keys = "ERROR: -mg nu=K,cs=K,limit=N,levels=K,scale=S,omega=W,coarsening=auto|grid|mis,cycle=v|w|k|kgcr,klev=N,smooth=0|1,pomega=X (0 < X < 2, with smooth=1),smoother=jacobi|cheb,degree=N (1..8),ratio=X (> 1),est=S (0..100),safety=X (>= 1) (the last four with smoother=cheb): cannot read \"%s\"\n";
            const auto digits = [](const std::string &t) { return t.find_first_not_of("0123456789") == std::string::npos; };
            while (std::getline(ss, item, ',')) {
                const size_t eq = item.find('=');
                const std::string k = item.substr(0, eq), v = eq == std::string::npos ? "" : item.substr(eq + 1);
                bool ok = !v.empty();
                if (k == "nu") p.nu = atoi(v.c_str());
                else if (k == "cs") p.coarse_sweeps = atoi(v.c_str());
                else if (k == "limit") p.coarse_limit = atoll(v.c_str());
                else if (k == "levels") p.max_levels = atoi(v.c_str());
                else if (k == "scale") p.coarse_scale = atof(v.c_str());
                else if (k == "omega") p.omega = atof(v.c_str());
                else if (k == "coarsening" && (v == "auto" || v == "grid" || v == "mis")) p.coarsening = v == "auto" ? 0 : v == "grid" ? 1 : 2;
                else if (k == "cycle" && (v == "v" || v == "w" || v == "k" || v == "kgcr"))
                    precond_mg_cycle().cycle = v == "v" ? BIS_MG_CYCLE_V : v == "w" ? BIS_MG_CYCLE_W : v == "k" ? BIS_MG_CYCLE_K : BIS_MG_CYCLE_K_GCR;
                else if (k == "klev" && v.find_first_not_of("0123456789") == std::string::npos) precond_mg_cycle().levels = atoi(v.c_str());
                else if (k == "smooth" && (v == "0" || v == "1")) precond_mg_smooth().smooth = v == "1";
                else if (k == "pomega" && atof(v.c_str()) > 0.0 && atof(v.c_str()) < 2.0) { precond_mg_smooth().pomega = atof(v.c_str()); pomega_item = item; }
                else if (k == "smoother" && (v == "jacobi" || v == "cheb"))
                    precond_mg_smoother().kind = v == "cheb" ? BIS_MG_SMOOTH_CHEBYSHEV : BIS_MG_SMOOTH_JACOBI;
                else if (k == "degree" && digits(v) && atoi(v.c_str()) >= 1 && atoi(v.c_str()) <= 8) { precond_mg_smoother().degree = atoi(v.c_str()); cheb_item = item; }
                else if (k == "ratio" && atof(v.c_str()) > 1.0 && std::isfinite(atof(v.c_str()))) { precond_mg_smoother().ratio = atof(v.c_str()); cheb_item = item; }
                else if (k == "est" && digits(v) && atoi(v.c_str()) <= 100) { precond_mg_smoother().est_steps = atoi(v.c_str()); cheb_item = item; }
                else if (k == "safety" && atof(v.c_str()) >= 1.0 && std::isfinite(atof(v.c_str()))) { precond_mg_smoother().safety = atof(v.c_str()); cheb_item = item; }
                else ok = false;
                if (!ok) {
                    fprintf(stderr, mg_keys, item.c_str());
                    exit(EXIT_FAILURE);
                }
            }
            if (!cheb_item.empty() && precond_mg_smoother().kind != BIS_MG_SMOOTH_CHEBYSHEV) { // a key of a smoother that is not chosen
                fprintf(stderr, mg_keys, cheb_item.c_str());
                exit(EXIT_FAILURE);
            }
            if (!pomega_item.empty() && !precond_mg_smooth().smooth) { // the factor of a prolongator that is not smoothed
                fprintf(stderr, mg_keys, pomega_item.c_str());
                exit(EXIT_FAILURE);
            }
        }
        else if (arg == "-unfused") a->unfused = true;
        else if (arg == "-hostscalars") a->host_scalars = true;
        else if (arg == "-trsv" && i + 1 < argc) {
            const std::string m = argv[++i];
            a->trsv_mode = m == "tiled" ? 1 : m == "level" ? 0 : m == "chain" ? 2 : m == "wave" ? 3 : -1;
        } else if (arg == "-grid" && i + 1 < argc) {
            a->grid_hint[3] = 1;
            if (sscanf(argv[++i], "%lld,%lld,%lld,%lld", &a->grid_hint[0], &a->grid_hint[1], &a->grid_hint[2], &a->grid_hint[3]) < 3) {
                fprintf(stderr, "ERROR: -grid NX,NY,NZ[,DOF]\n");
                exit(EXIT_FAILURE);
            }
        }
        else if (arg == "-perm" && i + 1 < argc) { a->perm_mode = argv[++i]; a->perm_given = true; }
        else if (arg == "-dump-perm" && i + 1 < argc) a->dump_perm = argv[++i];
        else if (arg == "-dump-x" && i + 1 < argc) a->dump_x = argv[++i];
        else if (arg == "-perm-host") a->perm_host = true;
        else if (arg == "-cache" && i + 1 < argc) a->crs_cache = argv[++i];
        else if (arg == "-dev" && i + 1 < argc) a->device = atoi(argv[++i]);
        else std::cout << "ERROR: assign_cli_inputs: Arguement \"" << arg << "\" not recongnized." << std::endl;
    }
    if (a->preconditioner == PrecondType::MG && a->method != SolverType::ConjugateGradient && a->method != SolverType::GMRES &&
        a->method != SolverType::BiCGSTAB && a->method != SolverType::FGMRES && a->method != SolverType::MINRES &&
        a->method != SolverType::IDR) {
        fprintf(stderr, "ERROR: -p mg needs a Krylov method: -cg, -gm or -bi\n");
        exit(EXIT_FAILURE);
    }
    if (a->preconditioner == PrecondType::BlockJacobi && a->method != SolverType::ConjugateGradient && a->method != SolverType::GMRES &&
        a->method != SolverType::BiCGSTAB && a->method != SolverType::FGMRES && a->method != SolverType::MINRES &&
        a->method != SolverType::IDR) {
        fprintf(stderr, "ERROR: -p bj needs a Krylov method: -cg, -gm, -fgm, -mr or -bi\n");
        exit(EXIT_FAILURE);
    }
    // a K-cycle changes with its right-hand side: left-preconditioned GMRES builds its basis for ONE operator M^-1 A, and there is no flexible GMRES here
    if (a->preconditioner == PrecondType::MG && a->method == SolverType::GMRES &&
        (precond_mg_cycle().cycle == BIS_MG_CYCLE_K || precond_mg_cycle().cycle == BIS_MG_CYCLE_K_GCR)) {
        fprintf(stderr, "ERROR: -mg cycle=k|kgcr is not a fixed preconditioner, which -gm (left-preconditioned GMRES, not flexible) assumes: "
                        "use -cg or -bi, or cycle=v|w\n");
        exit(EXIT_FAILURE);
    }
    // MINRES assumes one fixed symmetric positive definite M, as -gm assumes one fixed M
    if (a->preconditioner == PrecondType::MG && a->method == SolverType::MINRES &&
        (precond_mg_cycle().cycle == BIS_MG_CYCLE_K || precond_mg_cycle().cycle == BIS_MG_CYCLE_K_GCR)) {
        fprintf(stderr, "ERROR: -mg cycle=k|kgcr is not a fixed preconditioner, which -mr (MINRES) assumes: use -fgm, or cycle=v|w\n");
        exit(EXIT_FAILURE);
    }
    if (a->method == SolverType::MINRES && (a->unfused || a->host_scalars)) {
        fprintf(stderr, "ERROR: -mr is a device schedule (bis_minres_*) and has no call-by-call form: -unfused and -hostscalars do not apply\n");
        exit(EXIT_FAILURE);
    }
    // IDR(s) assumes one fixed M: its recurrences carry G_k = A M^-1 (...) from cycle to cycle
    if (a->preconditioner == PrecondType::MG && a->method == SolverType::IDR &&
        (precond_mg_cycle().cycle == BIS_MG_CYCLE_K || precond_mg_cycle().cycle == BIS_MG_CYCLE_K_GCR)) {
        fprintf(stderr, "ERROR: -mg cycle=k|kgcr is not a fixed preconditioner, which -idr (IDR(s)) assumes: use -fgm, or cycle=v|w\n");
        exit(EXIT_FAILURE);
    }
    if (a->method == SolverType::IDR && (a->unfused || a->host_scalars)) {
        fprintf(stderr, "ERROR: -idr is a device schedule (bis_idr_*) and has no call-by-call form: -unfused and -hostscalars do not apply\n");
        exit(EXIT_FAILURE);
    }
    if (a->ids_given && a->method != SolverType::IDR) {
        fprintf(stderr, "ERROR: -ids S is the dimension of the shadow space of IDR(s): it needs the method -idr\n");
        exit(EXIT_FAILURE);
    }
    if (a->method == SolverType::FGMRES && (a->unfused || a->host_scalars)) {
        fprintf(stderr, "ERROR: -fgm is a device schedule (bis_fgmres_*) and has no call-by-call form: -unfused and -hostscalars do not apply\n");
        exit(EXIT_FAILURE);
    }
    if (a->method == SolverType::LSMR) {
        // a rectangular system has no triangles to sweep, no symmetric permutation or scaling, and the handle is the only form
        const char *flag = a->precond_given ? "-p" : a->perm_given ? "-perm" : a->unfused ? "-unfused" : a->host_scalars ? "-hostscalars"
                           : a->num_scale ? "-scale 1" : nullptr;
        if (flag) {
            fprintf(stderr, "ERROR: %s does not apply to -lsmr (LSMR on the device schedule bis_lsmr_*: no preconditioner, permutation, "
                            "symmetric scaling or call-by-call form; use -colscale and -damp L)\n", flag);
            exit(EXIT_FAILURE);
        }
    } else if (a->damp_given || a->colscale) {
        fprintf(stderr, "ERROR: %s is an option of LSMR: it needs the method -lsmr\n", a->damp_given ? "-damp L" : "-colscale");
        exit(EXIT_FAILURE);
    }
    if (a->method == SolverType::Eigs) {
        // an eigenproblem has no right-hand side to precondition, the permutation and the scaling would change the vectors, and
        // the handle is the only form
        const char *flag = a->precond_given ? "-p" : a->perm_given ? "-perm" : a->scale_given ? "-scale" : a->unfused ? "-unfused"
                           : a->host_scalars ? "-hostscalars" : nullptr;
        if (flag) {
            fprintf(stderr, "ERROR: %s does not apply to -eig K (thick-restart Lanczos on the device schedule bis_eigs_*: no preconditioner, "
                            "permutation, scaling or call-by-call form; use -which sa|la|lm and -ncv M)\n", flag);
            exit(EXIT_FAILURE);
        }
        if (a->ncv_given && eigs_ncv() <= eigs_k()) {
            fprintf(stderr, "ERROR: -ncv M: the basis size of -eig K must exceed K\n");
            exit(EXIT_FAILURE);
        }
    } else if (a->method == SolverType::SVDS) {
        // singular triplets have no right-hand side to precondition, the permutation and the scaling would change the vectors,
        // and the handle is the only form
        const char *flag = a->precond_given ? "-p" : a->perm_given ? "-perm" : a->scale_given ? "-scale" : a->unfused ? "-unfused"
                           : a->host_scalars ? "-hostscalars" : nullptr;
        if (flag) {
            fprintf(stderr, "ERROR: %s does not apply to -svd K (thick-restart Lanczos bidiagonalisation on the device schedule bis_svds_*: no "
                            "preconditioner, permutation, scaling or call-by-call form; use -which lm|sm and -ncv M)\n", flag);
            exit(EXIT_FAILURE);
        }
        if (a->ncv_given && svds_ncv() <= svds_k()) {
            fprintf(stderr, "ERROR: -ncv M: the basis size of -svd K must exceed K\n");
            exit(EXIT_FAILURE);
        }
    } else if (a->which_given || a->ncv_given) {
        fprintf(stderr, "ERROR: %s is an option of the eigensolver: it needs the method -eig K\n", a->which_given ? "-which" : "-ncv M");
        exit(EXIT_FAILURE);
    }
    if (a->fill_given && a->preconditioner != PrecondType::ILU0 && a->preconditioner != PrecondType::ILU0Iter) {
        fprintf(stderr, "ERROR: -fill K is the level-of-fill of an incomplete LU factorisation: it needs -p ilu0 or -p ilu0it\n");
        exit(EXIT_FAILURE);
    }
    // the other types run exact sweeps on the fp64 arrays and would gain nothing from rounded values
    if (a->pprec == 32 && a->preconditioner != PrecondType::FSAI && a->preconditioner != PrecondType::ILU0Iter) {
        fprintf(stderr, "ERROR: -pprec 32 needs a preconditioner that is applied by SpMV: -p fsai or -p ilu0it\n");
        exit(EXIT_FAILURE);
    }
}

inline void print_timers(Args *cli_args, Timers *timers) {
    auto line = [&](const char *label, const char *key) {
        std::cout << std::left << std::setw(25) << label << std::right << std::setw(30)
                  << (*timers)[key].get_wtime() << "[s]" << std::endl;
    };
    const SolverType m = cli_args->method;
    std::cout << std::endl << std::scientific << std::setprecision(3);
    std::cout << "+---------------------------------------------------------+" << std::endl;
    line("Total elapsed time: ", "total");
    line("| Preprocessing time: ", "preprocessing");
    line("| | Init time: ", "preprocessing_init");
    line("| | Factor time: ", "preprocessing_factor");
    line("| Solve time: ", "solve");
    line("| | Iterate time: ", "iterate");
    line("| | | SpMV time: ", "spmv");
    line("| | | Precond. time: ", "precond");
    if (m == SolverType::Jacobi) line("| | | Normalize time: ", "normalize");
    else if (m == SolverType::GaussSeidel || m == SolverType::SymmetricGaussSeidel) {
        line("| | | Sum time: ", "sum");
        line("| | | SpTRSV time: ", "sptrsv");
    } else if (m == SolverType::ConjugateGradient || m == SolverType::BiCGSTAB) {
        line("| | | Dot time: ", "dot");
        line("| | | Sum time: ", "sum");
    } else if (m == SolverType::GMRES) {
        line("| | | Orthog. time: ", "orthog");
        line("| | | | Dot time: ", "dot");
        line("| | | | Sum time: ", "sum");
        line("| | | | Norm time: ", "norm");
        line("| | | | Scale time: ", "scale");
        line("| | | Least Sq. time: ", "least_sq");
        line("| | | | DGEMM time: ", "dgemm");
        line("| | | Update g time: ", "update_g");
        line("| | | | DGEMV time: ", "dgemv");
    }
    line("| | Sample time: ", "sample");
    line("| | Exchange time: ", "exchange");
    if (m == SolverType::GMRES) line("| | Restart time: ", "restart");
    line("| | Save x* time: ", "save_x_star");
    line("| Postprocessing time: ", "postprocessing");
    std::cout << "+---------------------------------------------------------+" << std::endl << std::endl;
}

inline void convert_coo_to_crs(MatrixCOO *coo, MatrixCRS *crs) {
    crs->n_rows = (int)coo->n_rows; crs->n_cols = (int)coo->n_cols; crs->nnz = coo->nnz;
    crs->row_ptr = new crs_index[crs->n_rows + 1]();
    crs->col = new int[crs->nnz ? crs->nnz : 1];
    crs->val = new double[crs->nnz ? crs->nnz : 1];
    for (crs_index k = 0; k < crs->nnz; ++k) { crs->col[k] = coo->J[k]; crs->val[k] = coo->values[k]; ++crs->row_ptr[coo->I[k] + 1]; }
    for (int r = 0; r < crs->n_rows; ++r) crs->row_ptr[r + 1] += crs->row_ptr[r];
    if (crs->row_ptr[crs->n_rows] != crs->nnz) { printf("ERROR: converting to CRS.\n"); exit(1); }
}

// Binary CRS cache of a parsed .mtx input: header {magic, n_rows, n_cols, nnz, size and
// modification time of the .mtx it was made from} as int64, then row_ptr (int64[n_rows+1]), col (int32[nnz]),
// val (double[nnz]) exactly as convert_coo_to_crs produced them, so a cached run sees the same matrix bit for bit.
// A cache that does not belong to the named .mtx (other size / time stamp), is truncated, or whose structure is
// not a CRS (row_ptr not monotone from 0 to nnz, column out of range) is ignored and rewritten.
inline bool source_stamp(const std::string &mtx, long long &size, long long &mtime) {
    struct stat st;
    if (stat(mtx.c_str(), &st) != 0) return false;
    size = (long long)st.st_size; mtime = (long long)st.st_mtime;
    return true;
}
inline bool read_crs_cache(const std::string &path, const std::string &mtx, MatrixCRS *A) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    long long h[6] = {0, 0, 0, 0, 0, 0}, sz = 0, mt = 0;
    bool ok = fread(h, sizeof(long long), 6, f) == 6 && h[0] == 0x4253435232ll && source_stamp(mtx, sz, mt) && h[4] == sz && h[5] == mt &&
              h[1] >= 0 && h[1] < INT32_MAX && h[2] == h[1] && h[3] >= 0;
    if (ok) { // the payload must be exactly what the header promises
        const long long want = 48 + 8 * (h[1] + 1) + 12 * h[3];
        struct stat st;
        ok = stat(path.c_str(), &st) == 0 && (long long)st.st_size == want;
    }
    if (ok) {
        MatrixCRS tmp((std::size_t)h[1], (std::size_t)h[2], (std::size_t)h[3]);
        ok = fread(tmp.row_ptr, sizeof(crs_index), (size_t)h[1] + 1, f) == (size_t)h[1] + 1 &&
             fread(tmp.col, sizeof(int), (size_t)h[3], f) == (size_t)h[3] &&
             fread(tmp.val, sizeof(double), (size_t)h[3], f) == (size_t)h[3];
        ok = ok && tmp.row_ptr[0] == 0 && tmp.row_ptr[h[1]] == h[3];
        for (long long r = 0; ok && r < h[1]; ++r) ok = tmp.row_ptr[r] <= tmp.row_ptr[r + 1];
        for (long long k = 0; ok && k < h[3]; ++k) ok = tmp.col[k] >= 0 && tmp.col[k] < h[2];
        if (ok) *A = tmp;
    }
    fclose(f);
    return ok;
}
inline void write_crs_cache(const std::string &path, const std::string &mtx, const MatrixCRS *A) {
    long long sz = 0, mt = 0;
    if (!source_stamp(mtx, sz, mt)) return;
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "WARNING: cannot write the CRS cache %s\n", path.c_str()); return; }
    const long long h[6] = {0x4253435232ll, A->n_rows, A->n_cols, A->nnz, sz, mt};
    fwrite(h, sizeof(long long), 6, f);
    fwrite(A->row_ptr, sizeof(crs_index), (size_t)A->n_rows + 1, f);
    fwrite(A->col, sizeof(int), (size_t)A->nnz, f);
    fwrite(A->val, sizeof(double), (size_t)A->nnz, f);
    fclose(f);
}

// generator strings -> device-resident matrix (no host copy)
inline bool make_generated_matrix(const std::string &spec, MatrixCRS *A) {
    auto split = [](const std::string &s, char d) {
        std::vector<std::string> out; std::stringstream ss(s); std::string t;
        while (std::getline(ss, t, d)) out.push_back(t);
        return out;
    };
    const auto head = split(spec, ':');
    if (head.size() != 2) return false;
    bis_mat *m = nullptr;
    const auto f = split(head[1], ',');
    if (head[0] == "hpcg") {
        long nx = atol(f[0].c_str()), ny = nx, nz = nx;
        if (f.size() == 3) { ny = atol(f[1].c_str()); nz = atol(f[2].c_str()); }
        bis::check(bis_mat_gen_hpcg(bis::ctx(), nx, ny, nz, 0, nx * ny * nz, &m), "bis_mat_gen_hpcg");
    } else if (head[0] == "anderson") {
        const long L = atol(f[0].c_str());
        double t = 1.0, W = 5.0, shift = 0.0;
        unsigned long long seed = 1;
        for (size_t i = 1; i < f.size(); ++i) {
            const auto kv = split(f[i], '=');
            if (kv.size() != 2) continue;
            if (kv[0] == "shift") shift = atof(kv[1].c_str());
            else if (kv[0] == "W") W = atof(kv[1].c_str());
            else if (kv[0] == "t") t = atof(kv[1].c_str());
            else if (kv[0] == "seed") seed = strtoull(kv[1].c_str(), nullptr, 10);
        }
        bis::check(bis_mat_gen_anderson(bis::ctx(), L, t, W, shift, seed, 0, L * L * L, &m), "bis_mat_gen_anderson");
    } else if (head[0] == "fem" || head[0] == "unstr") { // fem:NX[,NY,NZ][,keep=K][,seed=S]  (3 unknowns per node); unstr: the same
                                                          // under a seeded random row permutation, no grid (bis_mat_gen_unstr)
        long nx = atol(f[0].c_str()), ny = nx, nz = nx;
        int keep = 85;
        unsigned long long seed = 1;
        size_t i = 1;
        if (f.size() >= 3 && f[1].find('=') == std::string::npos && f[2].find('=') == std::string::npos) {
            ny = atol(f[1].c_str()); nz = atol(f[2].c_str()); i = 3;
        }
        for (; i < f.size(); ++i) {
            const auto kv = split(f[i], '=');
            if (kv.size() != 2) continue;
            if (kv[0] == "keep") keep = atoi(kv[1].c_str());
            else if (kv[0] == "seed") seed = strtoull(kv[1].c_str(), nullptr, 10);
        }
        if (head[0] == "unstr") bis::check(bis_mat_gen_unstr(bis::ctx(), nx, ny, nz, keep, seed, nullptr, &m), "bis_mat_gen_unstr");
        else bis::check(bis_mat_gen_fem(bis::ctx(), nx, ny, nz, keep, seed, 0, 3 * nx * ny * nz, &m), "bis_mat_gen_fem");
    } else return false;
    A->adopt(m);
    return true;
}
