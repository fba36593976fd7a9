/*
 * ecm2_pa.h -- C ABI of the MI355X-native PA diffusion+mass operator.
 *
 * This is the drop-in boundary for the reference's
 *   BilinearForm(PARTIAL) + MassIntegrator(alpha) + DiffusionIntegrator(beta)
 * hot path (PABilinearFormExtension, fem/bilinearform_ext.hpp:67-144).  Plain C:
 * opaque handles, plain pointers and sizes, int status codes (0 = ok), no HIP or
 * torch types.  Streams are passed as `void *` holding a hipStream_t (NULL = the
 * null stream, which is what the reference uses: general/forall.hpp:782).
 *
 * Memory: arguments documented "host" are read during the call; arguments
 * documented "device" are HBM pointers (hipMalloc / torch CUDA tensors).
 * Errors mirror MFEM_VERIFY -> mfem_error (general/error.cpp:154-184): the call
 * returns a nonzero ECM2_ERR_* code and ecm2_last_error() holds the message.
 * There is no CPU fallback: without a GPU every compute entry point fails with
 * ECM2_ERR_HIP.  See INTEGRATION.md for the reference-side binding.
 */
#ifndef ECM2_PA_H
#define ECM2_PA_H

#ifdef __cplusplus
extern "C" {
#endif

#define ECM2_OK 0
#define ECM2_ERR_ARG 1
#define ECM2_ERR_HIP 2
#define ECM2_ERR_STATE 3
#define ECM2_ERR_IO 4
#define ECM2_ERR_UNSUPPORTED 5
#define ECM2_ERR_COMM 6
#define ECM2_ERR_INTERNAL 7
#define ECM2_ERR_NUMERIC 8  /* a non-finite value where the reference's MFEM_VERIFY(IsFinite(..)) aborts
                              (CGSolver::Mult's nom / den / betanom, linalg/solvers.cpp:896, 932, 954, 993) */

/* Integrator kinds (MassIntegrator, DiffusionIntegrator: fem/bilininteg.hpp:2177-2465). */
#define ECM2_MASS 0
#define ECM2_DIFFUSION 1
/* ConvectionIntegrator(vel, alpha) (fem/bilininteg.hpp; PA: fem/integ/bilininteg_convection_pa.cpp): the
 * blood-flow advection rho_b c_b u . grad T of the bioheat operator, on the serial ecm2_pa_form.
 *   Setup   PAConvectionSetup3D (bilininteg_convection_pa.cpp:100-152): pa_data(q, c, e) =
 *           alpha W_q (adj J(q) v(q))_c, three values per point, reference layout [e][3][nq].
 *   Rule    ConvectionIntegrator::GetRule (fem/bilininteg.cpp:1610-1623, fem/eltrans.cpp:477-523): order
 *           2p + 2 on a trilinear hex = p + 2 points per direction, the form's default.  The form's rule
 *           must be p + 1 or p + 2 points with p = 1..4 (the reference's specialisations,
 *           bilininteg_convection_pa.cpp:30-58); otherwise add_integrator returns ECM2_ERR_UNSUPPORTED.
 *   Apply   PAConvectionApply3D (bilininteg_convection_kernels.hpp:274-451): y_e += B^T [(pa . grad_ref) x_e];
 *           transpose PAConvectionApplyT3D (:897-): y_e += sum_c G_c^T [pa_c (B x_e)].
 *   Coefficient: ECM2_COEFF_CONST_VECTOR (host data[3]) or ECM2_COEFF_QUAD_VECTOR (device [ne][nq][3], the
 *           velocity projected at the rule's points); params[0] = alpha, NULL = 1; any other kind is
 *           ECM2_ERR_ARG.  The qdata is built at assemble from the live array (assemble-time semantics).
 *   Markers (ecm2_pa_form_add_integrator_marked): the term acts on the marked attributes only (the fluid
 *           domain); only those active elements are stored and launched, a term with none launches nothing.
 *   Mult = volume part, boundary term, then C x: one apply into an E-vector over the active elements and a
 *           fixed-order add pass (no atomics; two Mults are bitwise equal).  ecm2_pa_form_mult_transpose
 *           adds C^T x instead.  AddMult, the ecm2_operator wrapper and the ODE steps follow.
 *   Diagonal: the reference aborts (AssembleDiagonalPA, bilininteg_convection_pa.cpp:216-227);
 *           ecm2_pa_form_assemble_diagonal returns ECM2_ERR_UNSUPPORTED on a form whose convection
 *           integrator has an active element, and so does ecm2_pcg_solve(jacobi = 1) on it.  Put the
 *           convection in the explicit operator K of ecm2_ode_step only: T = M + c dt K_sym stays symmetric.
 *           Or take it implicitly: ecm2_operator_bicgstab / ecm2_ode_step_bicgstab solve the nonsymmetric
 *           T = M + c dt (K_sym + C), with the Jacobi preconditioner built from the symmetric part.
 *   ecm2_pa_form_energy_parts is 0 for such a form.  At most one per form (a second: ECM2_ERR_UNSUPPORTED);
 *   distributed forms (ecm2_par_form_add_integrator[_marked]) return ECM2_ERR_UNSUPPORTED. */
#define ECM2_CONVECTION 2

/* Coefficient kinds (CoefficientVector COMPRESSED storage, fem/coefficient.cpp:2006-2180). */
#define ECM2_COEFF_CONSTANT 0       /* ConstantCoefficient                                   */
#define ECM2_COEFF_QUAD 1           /* values at quadrature points, device [ne][nq]          */
#define ECM2_COEFF_GRIDFUNC_AFFINE 2/* scale*(1+slope*(T(x_q)-t_ref)), T an H1 L-vector       */
/* Pennes heat capacity + perfusion of the implicit stage's mass coefficient, T an H1 L-vector:
 *   alpha(T) = rho_c + gdt_cb * w_b(T),  w_b(T) = w0 * max(0, 1 + a (T - t0)) for T < t_stop,
 *   0 at or above t_stop (perfusion shut-down in coagulated tissue);
 * params[0..5] = (rho_c, gdt_cb, w0, a, t0, t_stop).  T is projected to the quadrature points
 * like a GridFunctionCoefficient (qfunction.cpp:73-98, coefficient.cpp:2052-2070); the law
 * itself is the bioheat application's (not in the reference snapshot: parity-unpinned). */
#define ECM2_COEFF_GRIDFUNC_PERFUSION 3
/* Vector and matrix diffusion coefficients -- anisotropic (fibre-oriented) tissue conductivity;
 * DiffusionIntegrator(VectorCoefficient | MatrixCoefficient), PADiffusionSetup3D coeffDim 3 / 6 / 9
 * (fem/integ/bilininteg_diffusion_kernels.cpp:297-348), DiffusionIntegrator only.  QUAD_*: device
 * [ne][nq][dim]; CONST_*: host data[dim].  dim 3: diag(v); 6: symmetric (11,12,13,22,23,33)
 * (SymmetricMatrixCoefficient::ProjectSymmetric); 9: general, row-major M(i,j) at 3 i + j (the
 * transposed projection of CoefficientVector::ProjectTranspose, coefficient.cpp:2093-2123).  These
 * keep the full per-point layout (BLOCKED / NATIVE: 6 symmetric entries); a general matrix keeps
 * the reference's 9-entry qdata (ECM2_QLAYOUT_NATIVE9) and runs the workgroup-per-element or
 * unfused kernels (ECM2_ERR_UNSUPPORTED for ECM2_KERNEL_TPE / _LINE). */
#define ECM2_COEFF_QUAD_VECTOR 4
#define ECM2_COEFF_QUAD_SYMMATRIX 5
#define ECM2_COEFF_QUAD_MATRIX 6
#define ECM2_COEFF_CONST_VECTOR 7
#define ECM2_COEFF_CONST_SYMMATRIX 8
#define ECM2_COEFF_CONST_MATRIX 9
/* GridFunctionCoefficient of an H1 field on the form's own space (fem/coefficient.cpp:250-253 ->
 * QuadratureFunction::ProjectGridFunction, qfunction.cpp:73-98): data = the field's device L-vector,
 * params NULL; the value at a point is the interpolated field (no law) -- e.g. ex16p's conductivity
 * kappa + alpha u formed at the dofs, examples/ex16p.cpp:450-466. */
#define ECM2_COEFF_GRIDFUNC 10

/* Kernel selection (all produce the same operator). */
#define ECM2_KERNEL_AUTO 0     /* TPE for p <= 2, LINE for p = 3..6                 */
#define ECM2_KERNEL_TPE 1      /* fused, thread per element (p = 1, 2)              */
#define ECM2_KERNEL_WPE 2      /* fused, workgroup per element (p = 1..6)           */
#define ECM2_KERNEL_UNFUSED 3  /* reference-shaped: R, per-integrator AddMultPA, R^T */
#define ECM2_KERNEL_LINE 4     /* fused, one wave per element, register lines (p <= 6) */

/* Numbering of H1 dofs. */
#define ECM2_NUMBERING_ENTITY 0     /* vertices, edges, faces, interiors (fespace.cpp:2767) */
#define ECM2_NUMBERING_STRUCTURED 1 /* lattice numbering of a Cartesian mesh               */

const char *ecm2_last_error(void);
int ecm2_version(void);
int ecm2_device_count(void);
/* Measurement helper (no reference counterpart): b[0..n) = a[0..n) with 16-byte
 * nontemporal loads/stores -- the HBM STREAM-copy rate bench.py reports beside the
 * spec peak.  n even, a and b 16-byte aligned device arrays. */
int ecm2_stream_copy(const double *a, double *b, long n, void *stream);
/* Read-only HBM stream over a[0..n) (16-byte nontemporal loads, a per-thread sum written to
 * out[0..nout)): the read bandwidth the read-dominated PA kernels are measured against. */
int ecm2_stream_read(const double *a, long n, double *out, long nout, void *stream);

/* ------------------------------------------------------------------------ */
/* Setup side: meshes and H1 spaces (the caller's Mesh / FiniteElementSpace)  */
/* ------------------------------------------------------------------------ */
typedef struct ecm2_mesh ecm2_mesh;
typedef struct ecm2_h1space ecm2_h1space;

/* Mesh::MakeCartesian3D(..., sfc_ordering = false), mesh/mesh.cpp:3683 (lexicographic element order). */
int ecm2_mesh_cartesian(int nx, int ny, int nz, double sx, double sy, double sz, ecm2_mesh **out);
/* Mesh::MakeCartesian3D(nx, ny, nz, HEXAHEDRON, sx, sy, sz, sfc_ordering) (mesh.hpp:898-904,
 * mesh.cpp:3683-3813): sfc_ordering = 1 (the reference's default) orders the elements along
 * NCMesh::GridSfcOrdering3D's generalized Hilbert curve (ncmesh.cpp:5435-5634). */
int ecm2_mesh_cartesian_ex(int nx, int ny, int nz, double sx, double sy, double sz, int sfc_ordering,
                           ecm2_mesh **out);
/* Mesh(filename): MFEM mesh v1.0 hex meshes and MFEM INLINE hex meshes
 * (mesh/mesh_readers.cpp:1356-1506; INLINE = Make3D with sfc_ordering, :1506).  Host file read. */
int ecm2_mesh_read(const char *path, ecm2_mesh **out);
/* Mesh::UniformRefinement, mesh/mesh.cpp:11403 (hex: 1 -> 8; UniformRefinement3D_base's vertex
 * and child numbering, mesh.cpp:10155-10290, 10635-10705). */
int ecm2_mesh_refine_uniform(ecm2_mesh *m);
/* Mesh(const Mesh &), the copy constructor (mesh/mesh.hpp): an independent copy -- a hierarchy keeps the mesh
 * before and after ecm2_mesh_refine_uniform. */
int ecm2_mesh_copy(const ecm2_mesh *m, ecm2_mesh **out);
/* CoarseFineTransformations::embeddings (Mesh::GetRefinementTransforms, mesh/mesh.hpp) of the mesh that
 * ecm2_mesh_refine_uniform(coarse) produces: fine element e has parent e / 8 and sits at the parent's native corner
 * e % 8 (mesh.cpp:10635-10705); octant = ox + 2 oy + 4 oz is that corner in the parent's lexicographic frame. */
int ecm2_mesh_refinement_embedding(const ecm2_mesh *coarse, int *parent, int *octant /* host [8 ne_coarse] */);
int ecm2_mesh_info(const ecm2_mesh *m, int *nv, int *ne);
int ecm2_mesh_get_vertices(const ecm2_mesh *m, double *out /* host [nv][3] */);
int ecm2_mesh_set_vertices(ecm2_mesh *m, const double *in /* host [nv][3] */);
int ecm2_mesh_get_elements(const ecm2_mesh *m, int *out /* host [ne][8], native order */);
/* Element attributes (Mesh::GetAttribute / SetAttribute + SetAttributes, mesh.hpp), host [ne],
 * every attribute >= 1. */
int ecm2_mesh_get_attributes(const ecm2_mesh *m, int *out);
int ecm2_mesh_set_attributes(ecm2_mesh *m, const int *in);
/* Lexicographic corner coordinates, host out[ne][3][8]. */
int ecm2_mesh_get_element_nodes(const ecm2_mesh *m, double *out);
/* Boundary elements (Mesh::GetNBE / GetBdrElementVertices / GetBdrAttribute): quadrilaterals.
 * Mesh::Make3D's six sides in its order (mesh/mesh.cpp:3815-3949: attributes 1 bottom, 6 top, 5 left,
 * 3 right, 2 front, 4 back), the `boundary` section of a v1.0 file (geometry type 3 only, anything
 * else is ECM2_ERR_UNSUPPORTED), Mesh::GenerateBoundaryElements (mesh.cpp:2453-2500: the faces with
 * one element, attribute 1) for a file without one; refinement gives quad i the children
 * 4i..4i+3 with its attribute (mesh.cpp:10716-10764). */
int ecm2_mesh_boundary_info(const ecm2_mesh *m, int *nbe);
int ecm2_mesh_get_boundary(const ecm2_mesh *m, int *verts /* host [nbe][4], the quad's order */,
                           int *attr /* host [nbe] */);
int ecm2_mesh_set_boundary_attributes(ecm2_mesh *m, const int *attr /* host [nbe], every one >= 1 */);
/* Corners of the boundary quads in the quad's lexicographic frame (xi runs v0 -> v1, eta runs
 * v0 -> v3: the corners v0, v1, v3, v2), host out[nbe][3][4] -- the frame of
 * ecm2_h1space_get_boundary_map. */
int ecm2_mesh_get_boundary_nodes(const ecm2_mesh *m, double *out);
/* Physical coordinates of the Gauss-Legendre quadrature points of every element, host
 * out[ne][q1d^3][3] (q lexicographic, qx fastest): the points a FunctionCoefficient is
 * projected at (Coefficient::Project, fem/coefficient.cpp:52-70). */
int ecm2_mesh_quadrature_points(const ecm2_mesh *m, int q1d, double *out);
/* Same for a subset of elements (host elems[n]), out[n][q1d^3][3]. */
int ecm2_mesh_quadrature_points_subset(const ecm2_mesh *m, int q1d, const int *elems, int n,
                                       double *out);
/* Element order for the fused kernel: 0 native, 1 brick (Cartesian meshes: 4x4x4 bricks
 * first), 2 Morton order of centroids (any mesh).  perm host [ne]. */
int ecm2_mesh_element_order(const ecm2_mesh *m, int kind, int *perm);
void ecm2_mesh_destroy(ecm2_mesh *m);

/* H1_FECollection(order) + FiniteElementSpace: element->dof table in
 * lexicographic order (ElementRestriction gather_map, fem/restriction.cpp:26-107). */
int ecm2_h1space_create(const ecm2_mesh *m, int order, int numbering, ecm2_h1space **out);
int ecm2_h1space_info(const ecm2_h1space *s, int *ndofs, int *ne, int *nd);
int ecm2_h1space_get_gather_map(const ecm2_h1space *s, int *out /* host [ne][nd] */);
/* Essential true dofs for ess_bdr = all (GetEssentialTrueDofs): two-call pattern,
 * out may be NULL to query *count. */
/* Element order with 4x4x4 bricks of face-linked elements first (one per 64-lane wave of
 * the thread-per-element kernel), found from the element->dof map alone; any conforming
 * hex mesh (no reference counterpart: the reference applies elements independently,
 * fem/restriction.cpp:152-186).  perm host [ne]: internal position -> element.  Host only;
 * a PA form without an explicit order derives the same order at assemble. */
int ecm2_h1space_element_order(const ecm2_h1space *s, int *perm);
int ecm2_h1space_boundary_dofs(const ecm2_h1space *s, int *out, int *count);
/* FiniteElementSpace::GetEssentialTrueDofs(bdr_attr_is_ess, ...) (fem/fespace.cpp:548-571 GetEssentialVDofs,
 * :622- MarkerToList) for a conforming scalar space: the sorted, unique dofs of the boundary elements whose
 * attribute a has bdr_marker[a - 1] != 0 (host [n_marker]), from the space's boundary map and the boundary
 * attributes of its mesh as they are at the call (the space refers to the mesh it was created on, which must
 * be alive and not refined since).  Two-call pattern, as ecm2_h1space_boundary_dofs.  A boundary attribute above
 * n_marker: ECM2_ERR_ARG.  An all-ones marker gives what ecm2_h1space_boundary_dofs gives. */
int ecm2_h1space_essential_dofs(const ecm2_h1space *s, const int *bdr_marker, int n_marker, int *out, int *count);
int ecm2_h1space_dof_coords(const ecm2_h1space *s, const ecm2_mesh *m, double *out /* host [ndofs][3] */);
/* The dofs of every boundary element, host out[nbe][(order+1)^2], lexicographic in the quad's own
 * frame (see ecm2_mesh_get_boundary_nodes), taken from the adjacent element's row of the gather
 * map: the boundary FaceRestriction's map (bilinearform_ext.cpp:300-328) up to the frame. */
int ecm2_h1space_get_boundary_map(const ecm2_h1space *s, int *out);
void ecm2_h1space_destroy(ecm2_h1space *s);

/* ------------------------------------------------------------------------ */
/* The PA form: drop-in for PABilinearFormExtension of Mass + Diffusion       */
/* ------------------------------------------------------------------------ */
typedef struct ecm2_pa_form ecm2_pa_form;

/* Replaces BilinearForm::SetAssemblyLevel(PARTIAL) + FiniteElementSpace
 * ElementRestriction construction (bilinearform.cpp:109-136, restriction.cpp:26-107).
 * gather_map: host [ne][(order+1)^3], MFEM gather_map semantics (-1-gid = minus sign).
 * q1d <= 0 selects the reference default rule (Q1D = order+2). */
int ecm2_pa_form_create(int ne, int order, int ndofs, const int *gather_map, int q1d,
                        ecm2_pa_form **out);
/* Geometry from lexicographic element corners, host [ne][3][8] (trilinear hexes). */
int ecm2_pa_form_set_element_nodes(ecm2_pa_form *f, const double *enodes);
/* Geometry from GeometricFactors::JACOBIANS (mesh.cpp:15242 layout NQ x 3 x 3 x NE),
 * device pointer, must stay valid until ecm2_pa_form_assemble returns. */
int ecm2_pa_form_set_jacobians(ecm2_pa_form *f, const double *J);
/* Quadrature-data layout (ecm2_pa_form_info's *layout).  AFFINE: when every element is
 * a parallelepiped (checked on the corners given to set_element_nodes, or on the Jacobians) and
 * the diffusion integrator is present, the p <= 2 fused kernel stores the constant element geometry
 * adj(J) adj(J)^T / det J once per element and one (W beta, W alpha det J) pair per
 * quadrature point (W beta alone without a MassIntegrator; W alpha det J alone with the coefficient
 * snapshot below): the reference's pa_data values (bilininteg_diffusion_kernels.cpp:349-362,
 * bilininteg_mass_pa.cpp:76) up to rounding, 3.3x fewer bytes at p = 2 (3.5x at p = 4,
 * AFFINE_E: element-ordered, for the p >= 3 line / brick kernels).  On by default;
 * ecm2_pa_form_set_geometry_compression(f, 0) keeps the full per-point layout. */
#define ECM2_QLAYOUT_NATIVE 0
#define ECM2_QLAYOUT_BLOCKED 1
#define ECM2_QLAYOUT_AFFINE 2
#define ECM2_QLAYOUT_AFFINE_E 3  /* the same compression for the p >= 3 line / brick kernels */
/* TRILINEAR (p <= 2, elements not all parallelepipeds, geometry from corners or from Jacobians
 * that a trilinear map produces): the element's trilinear-map coefficients once per element plus
 * one (W beta / det J, W alpha det J) pair per point; the fused kernel evaluates J and adj(J) at
 * every quadrature point (the reference's setup algebra, never stored): the AFFINE layout's bytes
 * on a general mesh.  TRILINEAR_E: the same for the p >= 3 line / brick kernels.  Every
 * compressed layout also serves a diffusion-only form (one W beta [/ det J] value per point). */
#define ECM2_QLAYOUT_TRILINEAR 4
#define ECM2_QLAYOUT_NATIVE9 5   /* [e][9][nq] general D_ij (a nonsymmetric matrix coefficient)    */
#define ECM2_QLAYOUT_TRILINEAR_E 6
int ecm2_pa_form_set_geometry_compression(ecm2_pa_form *f, int on);
/* Coefficient snapshot (p = 2, AFFINE layout, every 64-element block a lattice brick, the
 * diffusion coefficient a grid-function kind -- ECM2_COEFF_GRIDFUNC, _GRIDFUNC_AFFINE or
 * _GRIDFUNC_PERFUSION -- without an attribute marker): Assemble keeps a copy of the field at its
 * dofs (with an affine / identity law applied there) and the fused kernel interpolates it at the
 * quadrature points and applies the law there (as TransformedCoefficient::Eval, coefficient.cpp:262),
 * instead of storing W beta per point (the reference evaluates the same coefficient at the points in
 * its setup, coefficient.cpp:2052-2070): 8 B per point fewer.  A MassIntegrator with a constant
 * coefficient or a grid-function law of the SAME field (the Pennes heat capacity + perfusion
 * alpha(T)) then stores one value per element instead of W alpha det J per point: no per-point
 * stream at all.  The snapshot is taken at Assemble (the reference's assemble-time semantics).  On
 * by default; ecm2_pa_form_coefficient_snapshot reports whether the last Assemble took it. */
int ecm2_pa_form_set_coefficient_snapshot(ecm2_pa_form *f, int on);
int ecm2_pa_form_coefficient_snapshot(const ecm2_pa_form *f, int *on);
/* Introspection of the last Assemble's snapshot (no reference counterpart; any output may be NULL):
 * *on as above; *mass_values 0 = no MassIntegrator, 1 = W alpha det J stored per point, 2 = one value
 * per element (constant or same-field mass law); *law_at_point 1 = the field itself is interpolated and
 * the laws applied at the point, 0 = an affine / identity law applied to the snapshot's dofs. */
int ecm2_pa_form_snapshot_info(const ecm2_pa_form *f, int *on, int *mass_values, int *law_at_point);
/* Introspection (no reference counterpart): the number of partial sums of x^T A x the form's Mult
 * writes when ecm2_pcg_solve folds CGSolver's den = (A d, d) (solvers.cpp:993) into it -- one per
 * workgroup of the coefficient-snapshot kernel -- or 0 when the solver runs the dot pass instead. */
int ecm2_pa_form_energy_parts(const ecm2_pa_form *f, int *parts);
/* Introspection (no reference counterpart): *on = 1 when the last Assemble found every element's
 * adj(J) adj(J)^T / det J diagonal (axis-aligned hexahedra) and the apply kernel uses it as a diagonal -- the
 * coefficient-snapshot kernel (p = 2) or the brick kernel (AFFINE_E, p >= 3) -- with the general product's
 * values, whose off-diagonal terms would add exact zeros. */
int ecm2_pa_form_flux_diagonal(const ecm2_pa_form *f, int *on);
/* BilinearForm::AddDomainIntegrator(new MassIntegrator(Q)) / DiffusionIntegrator(Q)
 * (bilinearform.cpp:231-242).  data: CONSTANT -> data[0] (host);
 * QUAD -> device [ne][nq]; GRIDFUNC_AFFINE -> device L-vector T with
 * params[0..2] = (scale, slope, t_ref).  Device arrays must stay valid until assemble. */
int ecm2_pa_form_add_integrator(ecm2_pa_form *f, int integrator, int coeff_kind,
                                const double *data, const double *params);
/* BilinearForm::AddDomainIntegrator(integ, elem_marker) (bilinearform.cpp:237-242): as
 * ecm2_pa_form_add_integrator, restricted to the elements whose attribute a has
 * marker[a - 1] != 0 (host marker[n_marker]; the reference's PABilinearFormExtension::
 * AddMultWithMarkers, bilinearform_ext.cpp:753-774,807-847, masks the integrator's E-vector
 * output; here its quadrature data is zeroed on the excluded elements at assemble: the same
 * operator, no extra pass per Mult).  Needs ecm2_pa_form_set_attributes before assemble. */
int ecm2_pa_form_add_integrator_marked(ecm2_pa_form *f, int integrator, int coeff_kind, const double *data,
                                       const double *params, const int *marker, int n_marker);
/* Introspection of a ConvectionIntegrator (any output may be NULL): *present 1 when the form has one;
 * *n_active the elements kept by the last assemble; *transpose_distinct 1 when MultTranspose differs
 * from Mult (an active convection term). */
int ecm2_pa_form_convection_info(const ecm2_pa_form *f, int *present, int *n_active, int *transpose_distinct);
/* Element attributes of the form's elements (the mesh's, host [ne], caller element order). */
int ecm2_pa_form_set_attributes(ecm2_pa_form *f, const int *attr);
/* Robin boundaries: BilinearForm::AddBoundaryIntegrator(new MassIntegrator(h)[, bdr_marker]) at
 * AssemblyLevel::PARTIAL.
 *   MassIntegrator::AssemblePABoundary (fem/integ/bilininteg_mass_pa.cpp:81-125): pa_data(q, f) =
 *     W_q c detJ_face(q, f) over the boundary faces, dim = 2, rule MassIntegrator::GetRule on the
 *     boundary quad (fem/bilininteg.cpp:1450-1462; order 2p + 1, OrderW = 1, fem/eltrans.cpp:493-507):
 *     p + 1 Gauss-Legendre points per direction;
 *   the 2D mass apply B^T D B and the 2D diagonal (bilininteg_mass_pa.cpp:127-169);
 *   PABilinearFormExtension (fem/bilinearform_ext.cpp): setup :300-328, :354; Mult's boundary block
 *     :625-675 (bdr_face_restrict_lex->Mult, AddMultWithMarkers over bdr_face_attributes :807-847,
 *     AddMultTransposeInPlace); AssembleDiagonal's boundary block :441-452;
 *   FaceGeometricFactors DETERMINANTS (mesh/mesh.cpp:15275-15334): |dx/dxi x dx/deta|.
 * set_boundary: bdr_map host [nbe][(order+1)^2] (the boundary FaceRestriction's map, e.g.
 * ecm2_h1space_get_boundary_map), bdr_attr host [nbe] (GetBdrFaceAttributes), bdr_nodes host
 * [nbe][3][4] lexicographic corners in the frame of bdr_map's rows (NULL when set_boundary_detj
 * follows); q1d <= 0 selects p + 1, and p + 1 and p + 2 are supported (else ECM2_ERR_UNSUPPORTED).
 * A distributed local form refuses it (ECM2_ERR_UNSUPPORTED).  set_boundary_detj: FaceGeometricFactors::
 * detJ, device [nbe][q1d^2], valid until assemble.  add_boundary_integrator: integrator ECM2_MASS only
 * (ECM2_DIFFUSION: ECM2_ERR_UNSUPPORTED); coeff_kind ECM2_COEFF_CONSTANT (data[0], host) or _QUAD
 * (device [nbe][q1d^2], boundary element order), other kinds ECM2_ERR_ARG; marker host [n_marker],
 * 0 / 1 per boundary attribute, NULL: every face.  The markers are folded into the face data at
 * assemble; only faces some integrator acts on are kept.  Mult (every kernel mode), AddMult,
 * MultTranspose, the operator wrapper, PCG and the ODE steps then include the term: one face apply
 * and a fixed-order add pass (no atomics) after the volume result; AssembleDiagonal adds the face
 * diagonal with the reference's shared-vector marker rule (:441-452).  ecm2_pa_form_energy_parts is 0
 * for such a form (the folded energy would miss the face term). */
int ecm2_pa_form_set_boundary(ecm2_pa_form *f, int nbe, const int *bdr_map, const int *bdr_attr,
                              const double *bdr_nodes, int q1d);
int ecm2_pa_form_set_boundary_detj(ecm2_pa_form *f, const double *detj);
int ecm2_pa_form_add_boundary_integrator(ecm2_pa_form *f, int integrator, int coeff_kind, const double *data,
                                         const int *marker, int n_marker);
/* pa_data of boundary integrator `index` (in the order added) in the reference's layout, host
 * out[nbe][q1d^2]; zeros on the faces its marker excludes.  After assemble. */
int ecm2_pa_form_get_boundary_qdata(ecm2_pa_form *f, int index, double *out, void *stream);
/* Introspection (any output may be NULL): boundary elements, boundary integrators, faces kept by
 * the last assemble, points per direction of the face rule. */
int ecm2_pa_form_boundary_info(const ecm2_pa_form *f, int *nbe, int *n_integrators, int *n_active, int *q1d);
int ecm2_pa_form_set_kernel(ecm2_pa_form *f, int kernel);
/* Scatter of the fused thread-per-element kernel (no reference counterpart: the
 * reference's ElementRestriction::MultTranspose, restriction.cpp:146-186, is the
 * deterministic CSR sum this replaces).  ECM2_SCATTER_PARTIALS (default): dofs held by
 * one element entry are stored directly, shared ones summed from per-entry partial
 * slots in a fixed order -- bitwise reproducible; ECM2_SCATTER_ATOMIC: FP64 atomics. */
#define ECM2_SCATTER_PARTIALS 0
#define ECM2_SCATTER_ATOMIC 1
int ecm2_pa_form_set_scatter(ecm2_pa_form *f, int mode);
/* Work grouping of the p >= 3 line-kernel family (no reference counterpart; the
 * reference applies each element independently, bilininteg_diffusion_kernels.hpp:989-1214):
 * bz = -1 default (2 x 2 x 1), 0 = per-element line kernel only, 1 = bricks of 2 x 2 x 1
 * elements, 2 = 2 x 2 x 2 (p = 3..6 with the default rule).  A brick is one workgroup; its
 * internal shared faces are summed in LDS in a fixed order (deterministic).  Bricks exist only
 * with ECM2_SCATTER_PARTIALS and both integrators; elements outside bricks use the line
 * kernel. */
int ecm2_pa_form_set_bricks(ecm2_pa_form *f, int bz);
/* After assemble: bricks formed and their depth (0 = none). */
int ecm2_pa_form_brick_info(const ecm2_pa_form *f, int *n_bricks, int *bz);
/* Scatter statistics after assemble: shared dofs and their partial slots. */
int ecm2_pa_form_scatter_info(const ecm2_pa_form *f, int *n_shared, long *n_slots);
/* After assemble: of the fused kernel's n_units units (p <= 2: 64-element blocks, p >= 3:
 * bricks), the `lattice` ones address their dofs arithmetically (a lattice-numbered region:
 * d = base + X sx + Y sy + Z sz with face-determined sharing, checked against the gather map;
 * the others read the map); n_runs = runs of the run-compressed summation plan.  The
 * operator is the same either way. */
int ecm2_pa_form_addressing_info(const ecm2_pa_form *f, int *lattice, int *n_units, long *n_runs);
/* Summation-plan details (introspection): units whose partial slots are face-grouped although
 * their dofs are read from the map (non-lattice numberings, e.g. the reference's entity
 * numbering), and runs whose dofs come from the plan's entry list. */
int ecm2_pa_form_plan_info(const ecm2_pa_form *f, int *lattice_slot_units, long *n_explicit_runs);
/* Optional element permutation for the fused kernel's blocked layout (host perm[ne]:
 * internal position i <- caller element perm[i]); see ecm2_mesh_element_order.  All
 * entry points keep the caller's element order (the reference's E-vector order,
 * restriction.cpp:26-107, is never exposed differently). */
int ecm2_pa_form_set_element_order(ecm2_pa_form *f, const int *perm);
/* BilinearForm::Assemble -> PABilinearFormExtension::Assemble -> AssemblePA
 * (bilinearform.cpp:456-460, bilinearform_ext.cpp:332-368). */
int ecm2_pa_form_assemble(ecm2_pa_form *f, void *stream);
/* BilinearForm::Mult / PABilinearFormExtension::Mult (bilinearform.cpp:1244-1254,
 * bilinearform_ext.cpp:487-564): y = A x, y overwritten.  x, y device [ndofs]. */
int ecm2_pa_form_mult(ecm2_pa_form *f, const double *x, double *y, void *stream);
/* PABilinearFormExtension::MultTranspose (bilinearform_ext.hpp:99, bilinearform_ext.cpp:
 * 679-): y = A^T x.  Mass, Diffusion and the boundary mass are symmetric, so without a
 * ConvectionIntegrator this is the Mult, launch for launch (tests/test_gpu_parity.py asserts the
 * equality); with one, the volume and boundary parts as Mult plus C^T x (PAConvectionApplyT3D). */
int ecm2_pa_form_mult_transpose(ecm2_pa_form *f, const double *x, double *y, void *stream);
/* Operator::AddMult (linalg/operator.hpp:108-109): y += a A x. */
int ecm2_pa_form_add_mult(ecm2_pa_form *f, const double *x, double *y, double a, void *stream);
/* PABilinearFormExtension::AssembleDiagonal (bilinearform_ext.cpp:370-454). diag device [ndofs]. */
int ecm2_pa_form_assemble_diagonal(ecm2_pa_form *f, double *diag, void *stream);
/* ElementRestriction::Mult / MultTranspose (restriction.cpp:109-186). xe device [ne][nd]. */
int ecm2_pa_form_restriction_mult(ecm2_pa_form *f, const double *x, double *xe, void *stream);
int ecm2_pa_form_restriction_mult_transpose(ecm2_pa_form *f, const double *xe, double *y, void *stream);
/* BilinearFormIntegrator::AddMultPA (bilininteg.hpp:49-97): ye += A_integ xe (E-vectors). */
int ecm2_pa_form_integrator_add_mult(ecm2_pa_form *f, int integrator, const double *xe,
                                     double *ye, void *stream);
/* BilinearFormIntegrator::AddMultTransposePA (bilininteg.hpp:49-97): ye += A_integ^T xe.  For the
 * symmetric mass and diffusion it is the plain apply. */
int ecm2_pa_form_integrator_add_mult_transpose(ecm2_pa_form *f, int integrator, const double *xe,
                                               double *ye, void *stream);
/* pa_data in the reference layout (diffusion [ne][6][nq], mass [ne][nq], convection [ne][3][nq] with
 * zeros on the elements its marker excludes), host out. */
int ecm2_pa_form_get_qdata(ecm2_pa_form *f, int integrator, double *out, void *stream);
int ecm2_pa_form_info(const ecm2_pa_form *f, int *ne, int *ndofs, int *d1d, int *q1d,
                      int *kernel, int *layout);
/* HIP-event timing of the dominant apply kernel(s) inside Mult. */
int ecm2_pa_form_timing(ecm2_pa_form *f, int enable);
int ecm2_pa_form_timing_get(ecm2_pa_form *f, double *total_ms, long *launches);
/* SURVEY §8(d) algorithmic bytes per Mult: 8*NE*NQ*(6+1) + 16*ndofs + 4*NE*ND. */
int ecm2_pa_form_algorithmic_bytes(const ecm2_pa_form *f, double *bytes);
/* Bytes of quadrature data the form stores after assemble (diffusion + mass). */
int ecm2_pa_form_qdata_bytes(const ecm2_pa_form *f, double *bytes);
/* ~PABilinearFormExtension / BilinearForm::Update (bilinearform_ext.hpp:67-144). */
void ecm2_pa_form_destroy(ecm2_pa_form *f);

/* ------------------------------------------------------------------------ */
/* Caller: constrained Jacobi-PCG (ConstrainedOperator operator.cpp:586-646 + */
/* CGSolver::Mult solvers.cpp:869-1004)                                       */
/* ------------------------------------------------------------------------ */
/* ess: device int [n_ess] essential dofs (DIAG_ONE).  b, x device [ndofs];
 * x is overwritten (iterative_mode = false) and must be 16-byte aligned (the update kernels move two
 * entries per access; a view at an odd element offset returns ECM2_ERR_ARG before anything is
 * enqueued).  jacobi != 0 -> OperatorJacobiSmoother.
 * iterations = CGSolver's final_iter, final_norm = sqrt((B r, r)) (the raw (B r, r) when it is
 * negative).  CGSolver's stops: converged, max_iter, (B r, r) < 0 or (A d, d) == 0 (not
 * converged: ecm2_pcg_last_converged() == 0); a non-finite (B r, r) or (A d, d), where the
 * reference's MFEM_VERIFY aborts, returns ECM2_ERR_NUMERIC. */
int ecm2_pcg_solve(ecm2_pa_form *f, const int *ess, int n_ess, const double *b, double *x,
                   double rel_tol, double abs_tol, int max_iter, int jacobi, int *iterations,
                   double *final_norm, void *stream);
/* IterativeSolver::GetConverged() (solvers.hpp:155) of the calling thread's last
 * ecm2_pcg_solve / ecm2_operator_pcg: 1 converged, 0 not (or no solve yet). */
int ecm2_pcg_last_converged(void);

/* ------------------------------------------------------------------------ */
/* Operators for the solvers: the serial form, one rank of the RCCL form, or */
/* the in-process loopback group (concatenated true vectors), all seen as the */
/* reference's Operator (linalg/operator.hpp:24-110) by PCG and the ODE step. */
/* ------------------------------------------------------------------------ */
typedef struct ecm2_operator ecm2_operator;
typedef struct ecm2_par_form ecm2_par_form;
/* The operator keeps a reference to the form(s): destroy it first. */
int ecm2_operator_from_pa_form(ecm2_pa_form *f, ecm2_operator **out);
int ecm2_operator_from_par_form(ecm2_par_form *f, ecm2_operator **out);
/* forms[r] must be rank r of an n-rank partition; vectors are the concatenation of the
 * ranks' true vectors (rank r at offset sum_{q<r} n_owned(q)). */
int ecm2_operator_from_par_group(ecm2_par_form *const *forms, int n, ecm2_operator **out);
/* Measurement (no reference counterpart): member `member` of the loopback group as one rank's
 * operator on its own GPU -- Mult = ecm2_par_group_mult_member (the peers' x held at zero in a
 * private buffer), dots summed by ncclAllReduce on a one-rank communicator.  Vectors are the
 * member's true dofs; ecm2_operator_pcg on it times one rank's solver iteration.  OVERLAP
 * decomposition with contiguous sends (slabs) only: ECM2_ERR_UNSUPPORTED otherwise. */
int ecm2_operator_from_par_member(ecm2_par_form *const *forms, int n, int member, ecm2_operator **out);
/* Operator::Height/Width and Operator::Mult (operator.hpp:24-110). */
int ecm2_operator_size(const ecm2_operator *op, int *n);
int ecm2_operator_mult(ecm2_operator *op, const double *x, double *y, void *stream);
/* ConstrainedOperator (operator.cpp:586-646) + CGSolver::Mult (solvers.cpp:869-1004) +
 * OperatorJacobiSmoother on any operator; with the RCCL form every rank calls it
 * collectively (dots are summed with ncclAllReduce, as the reference's parallel
 * InnerProduct sums with MPI_Allreduce).  x must be 16-byte aligned, as for ecm2_pcg_solve
 * (ECM2_ERR_ARG otherwise, before anything is enqueued). */
int ecm2_operator_pcg(ecm2_operator *op, const int *ess, int n_ess, const double *b, double *x,
                      double rel_tol, double abs_tol, int max_iter, int jacobi, int *iterations,
                      double *final_norm, void *stream);
/* ecm2_operator_pcg with IterativeSolver::iterative_mode (linalg/solvers.cpp:29-30: the reference's default is
 * true; ecm2_operator_pcg is this function with 0).  iterative_mode != 0: x is the start and is not cleared,
 * r = b - A~ x (CGSolver::Mult, solvers.cpp:875-884) by the constrained Mult, which zeroes and restores the
 * essential entries of x in place, and one 16-byte pass; b must then be 16-byte aligned too (ECM2_ERR_ARG).
 * Every stop, read-back and result after that is ecm2_operator_pcg's.  With b[ess] = x[ess], as
 * ecm2_operator_form_linear_system leaves them, r[ess] = 0 exactly and x[ess] keeps its bits.  The
 * preconditioner stays iterative_mode = false (solvers.cpp:181).  Every operator ecm2_operator_pcg accepts. */
int ecm2_operator_pcg_ex(ecm2_operator *op, const int *ess, int n_ess, const double *b, double *x,
                         double rel_tol, double abs_tol, int max_iter, int jacobi, int *iterations,
                         double *final_norm, void *stream, int iterative_mode);
/* ConstrainedOperator::EliminateRHS (linalg/operator.cpp:559-584), per entry: w = 0; w[ess] = x[ess]; z = A w;
 * b -= z; b[ess] = x[ess].  ess: device int [n_ess], sorted and unique; x, b: device vectors of the operator's
 * size, 16-byte aligned and distinct (ECM2_ERR_ARG otherwise, before anything is enqueued).  Any operator: the
 * serial form, a loopback group in its concatenated numbering, an RCCL rank or a member (the Mult is collective:
 * every rank calls it, one without essential dofs too).  w and z are the solvers' work vectors: nothing is
 * allocated after the first call of a size.  n_ess == 0 on an operator that does not communicate leaves b
 * bitwise unchanged and launches no kernel.  Returns with the stream synchronised. */
int ecm2_operator_eliminate_rhs(ecm2_operator *A, const int *ess, int n_ess, const double *x, double *b,
                                void *stream);
/* Operator::FormLinearSystem (linalg/operator.cpp:114-129) for the identity prolongation, in place (X = x,
 * B = b): with copy_interior == 0 the entries of x off the list are set to zero first
 * (X.SetSubVectorComplement(ess, 0.0)); then ecm2_operator_eliminate_rhs.  x carries the essential values in
 * and out; solve with iterative_mode = 1 (or 0: the solvers keep x[ess] = b[ess]).  Operator::RecoverFEMSolution
 * (operator.cpp:148-161) is the identity here: x is the solution. */
int ecm2_operator_form_linear_system(ecm2_operator *A, const int *ess, int n_ess, double *x, double *b,
                                     int copy_interior, void *stream);
/* ODESolver::SelectImplicit types (ode.cpp:77-91): 21 BackwardEuler, 22 SDIRK23 (L-stable),
 * 23 SDIRK33, 32 ImplicitMidpoint, 33 SDIRK23 (A-stable), 34 SDIRK34.  Returns the stage
 * coefficient c (every stage solves (M + c*dt*K) k = -K u_stage), 0 for unknown types. */
double ecm2_ode_implicit_coeff(int type);
/* One step of M du/dt = -K u (ex16 ConductionOperator::ImplicitSolve, ex16.cpp:327-354, in
 * the slope form; the SDIRK stage algebra of ode.cpp:682-859).  T must be assembled as
 * M + c*dt*K with c = ecm2_ode_implicit_coeff(type); u (device, true dofs) is advanced in
 * place; ess dofs keep their values.  Stage solves: constrained Jacobi-PCG (rel_tol,
 * max_iter).  *converged = 0 if some stage solve stopped at max_iter (like CGSolver, not an
 * error). */
int ecm2_ode_step(int type, ecm2_operator *T, ecm2_operator *K, double dt, double *u, const int *ess,
                  int n_ess, double rel_tol, int max_iter, int jacobi, int *solves, int *iterations,
                  int *converged, void *stream);
/* ecm2_ode_step with a source: one step of M du/dt = -K u + b, b a device true-dof vector in the
 * operator's own numbering (serial form, RCCL rank or loopback group alike), frozen over the step
 * (a TimeDependentOperator whose ImplicitSolve adds a LinearForm's vector to the right-hand side,
 * as the Joule miniapp's heat solve adds its DomainLFIntegrator(Wcoeff) form, joule_solver.cpp:
 * 401-, 616): every stage solves
 * T k = -K u_stage + b with the essential rows zeroed.  b == NULL is exactly ecm2_ode_step. */
int ecm2_ode_step_source(int type, ecm2_operator *T, ecm2_operator *K, const double *b, double dt, double *u,
                         const int *ess, int n_ess, double rel_tol, int max_iter, int jacobi, int *solves,
                         int *iterations, int *converged, void *stream);
/* ConstrainedOperator (operator.cpp:586-646) + BiCGSTABSolver::Mult (linalg/solvers.cpp:1579-1805) for a
 * nonsymmetric operator (a form with a ConvectionIntegrator), iterative_mode = false: x is overwritten
 * and must be 16-byte aligned (ECM2_ERR_ARG otherwise, before anything is enqueued).
 * jacobi_of (NULL: no preconditioner): OperatorJacobiSmoother built from a second operator of A's size
 * (ECM2_ERR_ARG otherwise), dinv = 1 / diag(jacobi_of) with the essential rows 1 -- as an MFEM user builds
 * it from the symmetric form, since the diagonal of a form with an active convection integrator is refused.
 * The reference's operations per entry and its stops, on norms: tol_goal = max(||r_0|| rel_tol, abs_tol);
 * ||r_0|| <= tol_goal converges with 0 iterations; ||s|| < tol_goal converges after x += alpha phat;
 * ||r|| < tol_goal converges; rho_1 == 0, omega == 0 and max_iter stop not converged
 * (ecm2_bicgstab_last_converged() == 0).  iterations = final_iter, final_norm = the last ||s|| or ||r||.
 * A non-finite ||r_0||, ||s|| or ||r|| (alpha = rho_1 / 0 included), where MFEM_VERIFY aborts, returns
 * ECM2_ERR_NUMERIC.  Serial forms and loopback groups; an operator whose dots need communication (an
 * RCCL rank, a group member) returns ECM2_ERR_UNSUPPORTED.  Two solves are bitwise equal. */
int ecm2_operator_bicgstab(ecm2_operator *A, ecm2_operator *jacobi_of /* NULL: none */, const int *ess, int n_ess,
                           const double *b, double *x, double rel_tol, double abs_tol, int max_iter,
                           int *iterations, double *final_norm, void *stream);
/* ecm2_operator_bicgstab with iterative_mode (ecm2_operator_bicgstab is this function with 0): != 0 starts from
 * the caller's x, r = b - A~ x, r~ = r (BiCGSTABSolver::Mult, linalg/solvers.cpp:1618-1622); b must then be
 * 16-byte aligned too (ECM2_ERR_ARG).  Nothing else changes. */
int ecm2_operator_bicgstab_ex(ecm2_operator *A, ecm2_operator *jacobi_of /* NULL: none */, const int *ess, int n_ess,
                              const double *b, double *x, double rel_tol, double abs_tol, int max_iter,
                              int *iterations, double *final_norm, void *stream, int iterative_mode);
/* IterativeSolver::GetConverged() of the calling thread's last ecm2_operator_bicgstab (BiCGSTABSolver,
 * linalg/solvers.cpp:1579-1805): 1 converged, 0 not (or no solve yet); per calling thread, as
 * ecm2_pcg_last_converged. */
int ecm2_bicgstab_last_converged(void);
/* ecm2_ode_step_source with the advection implicit: the stage solves run BiCGSTABSolver (linalg/solvers.cpp:
 * 1579-1805) instead of the PCG.  The caller assembles T = M + c*dt*(K_sym + C) and K = K_sym + C (the
 * ConvectionIntegrator inside both) and passes jacobi_of = M + c*dt*K_sym (NULL: no preconditioner); every
 * stage solves T k = -K u_stage [+ b] with the essential rows zeroed.  b == NULL: no source. */
int ecm2_ode_step_bicgstab(int type, ecm2_operator *T, ecm2_operator *jacobi_of, ecm2_operator *K, const double *b /* NULL */,
                           double dt, double *u, const int *ess, int n_ess, double rel_tol, int max_iter,
                           int *solves, int *iterations, int *converged, void *stream);

/* ------------------------------------------------------------------------ */
/* OperatorChebyshevSmoother (linalg/solvers.hpp:498-586, solvers.cpp:455-658), */
/* its eigenvalue estimate (PowerMethod::EstimateLargestEigenvalue,            */
/* linalg/operator.cpp:871-928) and CGSolver::Mult (solvers.cpp:869-1004) with */
/* the smoother as its preconditioner                                          */
/* ------------------------------------------------------------------------ */
/* The smoother y = sum_{k < order} c_k (D^-1 A~)^k D^-1 x on the DIAG_ONE constrained operator A~ (ess: device
 * int [n_ess], copied), D the diagonal of diag_of (NULL: of A; an operator of A's size, ECM2_ERR_ARG otherwise,
 * as ecm2_operator_bicgstab's jacobi_of) with the essential rows 1.  The diagonal is taken here: a form that is
 * assembled again needs a new smoother.  A (and diag_of) must outlive it.  order 1..5 (Setup,
 * solvers.cpp:538-617; any other: ECM2_ERR_ARG, where the reference aborts).  Serial forms and loopback groups;
 * an operator whose dots need communication (an RCCL rank, a group member): ECM2_ERR_UNSUPPORTED. */
typedef struct ecm2_smoother ecm2_smoother;
/* OperatorChebyshevSmoother(oper, d, ess_tdofs, order, max_eig_estimate) (solvers.cpp:455-469). */
int ecm2_chebyshev_create(ecm2_operator *A, ecm2_operator *diag_of /* NULL: A */, const int *ess, int n_ess, int order,
                          double max_eig_estimate, ecm2_smoother **out, void *stream);
/* OperatorChebyshevSmoother(oper, d, ess_tdofs, order, power_iterations, power_tolerance) (solvers.cpp:480-514;
 * the reference's defaults 10 and 1e-8): max_eig from ecm2_power_method (operator.cpp:871-928) on D^-1 A~.  v0 (device, 16-byte aligned,
 * or NULL): as ecm2_power_method's. */
int ecm2_chebyshev_create_power(ecm2_operator *A, ecm2_operator *diag_of /* NULL: A */, const int *ess, int n_ess,
                                int order, int power_iterations, double power_tolerance, double *v0 /* NULL */,
                                ecm2_smoother **out, void *stream);
/* order, the eigenvalue estimate, the power steps run (0: the estimate was given) and the coefficients
 * c_0 .. c_{order-1} (the rest 0) of Setup (solvers.cpp:538-617); any pointer may be NULL. */
int ecm2_chebyshev_info(const ecm2_smoother *sm, int *order, double *max_eig, int *power_steps, double coeffs[5]);
/* OperatorChebyshevSmoother::Mult (solvers.cpp:619-658), iterative_mode = false: y = S x, x and y distinct device
 * vectors of the operator's size, 16-byte aligned (ECM2_ERR_ARG otherwise).  Two calls are bitwise equal. */
int ecm2_chebyshev_mult(ecm2_smoother *sm, const double *x, double *y, void *stream);
void ecm2_smoother_destroy(ecm2_smoother *sm);
/* PowerMethod::EstimateLargestEigenvalue (linalg/operator.cpp:871-928) on D^-1 A~ (A~, D as above), seed = 0:
 * v0 (device, A's size, 16-byte aligned) holds the start vector on entry and the last iterate on return; NULL:
 * the library's own start vector, an integer hash of the index in (0, 1) (the reference's seeded glibc rand()
 * is not reproduced).  At most num_steps steps, ended when |(eig_new - eig) / eig| < tol (eig starts at 1);
 * *steps = the steps run.  A non-finite eigenvalue: ECM2_ERR_NUMERIC. */
int ecm2_power_method(ecm2_operator *A, ecm2_operator *diag_of /* NULL: A */, const int *ess, int n_ess,
                      double *v0 /* in: start, out: last iterate; NULL */, int num_steps, double tol, double *eig,
                      int *steps, void *stream);
/* ecm2_operator_pcg with prec = the smoother (CGSolver::Mult, solvers.cpp:869-1004; the smoother of A's size,
 * ECM2_ERR_ARG otherwise): the same stops, read-backs and results as there -- (B r, r) < 0 before the loop
 * (0 iterations, final_norm = the negative (B r, r)) or inside it and (A d, d) == 0 stop not converged; a
 * non-finite (B r, r) or (A d, d) returns ECM2_ERR_NUMERIC.  ecm2_pcg_last_converged reports it.  x must be
 * 16-byte aligned (ECM2_ERR_ARG).  Operators whose dots need communication: ECM2_ERR_UNSUPPORTED. */
int ecm2_operator_pcg_prec(ecm2_operator *A, ecm2_smoother *sm, const int *ess, int n_ess, const double *b, double *x,
                           double rel_tol, double abs_tol, int max_iter, int *iterations, double *final_norm,
                           void *stream);
/* ecm2_operator_pcg_prec with iterative_mode, as ecm2_operator_pcg_ex (CGSolver::Mult, solvers.cpp:875-884): the
 * outer CG starts from x; the smoother itself stays iterative_mode = false (solvers.cpp:181).  0: that function. */
int ecm2_operator_pcg_prec_ex(ecm2_operator *A, ecm2_smoother *sm, const int *ess, int n_ess, const double *b,
                              double *x, double rel_tol, double abs_tol, int max_iter, int *iterations,
                              double *final_norm, void *stream, int iterative_mode);
/* ecm2_ode_step_source whose stage solves run ecm2_operator_pcg_prec with sm, a smoother built from T (fixed
 * over the step, so one smoother serves every stage; CGSolver::Mult solvers.cpp:869-1004 with
 * OperatorChebyshevSmoother::Mult solvers.cpp:619-658).  b == NULL: no source. */
int ecm2_ode_step_prec(int type, ecm2_operator *T, ecm2_operator *K, const double *b /* NULL */, ecm2_smoother *sm,
                       double dt, double *u, const int *ess, int n_ess, double rel_tol, int max_iter, int *solves,
                       int *iterations, int *converged, void *stream);

/* ------------------------------------------------------------------------ */
/* p-multigrid: TensorProductPRefinementTransferOperator (fem/transfer.cpp:   */
/* 2223-2592), Multigrid's V-cycle (fem/multigrid.cpp:106-232) and            */
/* CGSolver::Mult (linalg/solvers.cpp:869-1004) with the cycle as prec        */
/* ------------------------------------------------------------------------ */
/* TensorProductPRefinementTransferOperator(lFESpace, hFESpace) (fem/transfer.cpp:2223-2287) between two H1 spaces
 * of orders order_lo < order_hi on the same ne elements in the same element order, each given by its gather map
 * (host int [ne][(order + 1)^3], lexicographic local dofs, as ecm2_pa_form_create's); nothing else about the
 * spaces is read.  The mask (ElementRestriction::BooleanMask, fem/restriction.cpp:248-283) is built here as owner
 * bits.  order_lo >= order_hi: ECM2_ERR_ARG; an order outside 1..4: ECM2_ERR_UNSUPPORTED; a map entry >= ndofs or
 * a fine dof that no element holds: ECM2_ERR_ARG; a negative (signed) entry: ECM2_ERR_UNSUPPORTED. */
typedef struct ecm2_transfer ecm2_transfer;
int ecm2_transfer_create(int ne, int order_lo, int ndofs_lo, const int *gather_lo, int order_hi, int ndofs_hi,
                         const int *gather_hi, ecm2_transfer **out);
/* FiniteElementSpace::RefinementOperator (fem/fespace.cpp:1833-2120; local matrices GetLocalRefinementMatrices
 * :1786-1807; what TransferOperator selects between two meshes, fem/transfer.cpp:2055-): the transfer between an H1
 * space on a hex mesh (ne_lo elements) and the H1 space of the same order (1..4) on its uniform refinement (ne_hi = 8
 * ne_lo), each given by its gather map, and the embedding of every fine element (host int [ne_hi]): its parent
 * and its octant ox + 2 oy + 4 oz in the parent's lexicographic frame (ecm2_mesh_refinement_embedding).  Nothing
 * else about the meshes is read.  The handle is ecm2_transfer_create's: ecm2_transfer_mult, _mult_transpose,
 * _info, _destroy and ecm2_multigrid_create take it unchanged; _info reports order_lo = order_hi and ne = ne_hi.
 * A null map or embedding, a map entry >= ndofs, a fine dof that no element holds, a parent or octant out of
 * range: ECM2_ERR_ARG; an order outside 1..4, a negative (signed) entry, a parent without exactly one child per
 * octant (non-conforming or partial refinement): ECM2_ERR_UNSUPPORTED. */
int ecm2_transfer_create_h(int order, int ne_lo, int ndofs_lo, const int *gather_lo, int ne_hi, int ndofs_hi,
                           const int *gather_hi, const int *parent, const int *octant, ecm2_transfer **out);
/* Mult (fem/transfer.cpp:2542-2566, Prolongation3D :2338-2423): y_hi = P x_lo, device L-vectors of ndofs_lo and
 * ndofs_hi doubles; y_hi is overwritten, every entry once by its owner element (no zero fill, no atomics). */
int ecm2_transfer_mult(ecm2_transfer *t, const double *x_lo, double *y_hi, void *stream);
/* MultTranspose (fem/transfer.cpp:2568-2592, Restriction3D :2470-2539): y_lo = P^T x_hi, summed over the elements
 * that share a coarse dof in a fixed order (no atomics); y_lo is overwritten.  Two calls are bitwise equal. */
int ecm2_transfer_mult_transpose(ecm2_transfer *t, const double *x_hi, double *y_lo, void *stream);
/* ne, the two orders and sizes, and the bytes of the device plan (both maps, the owner words, the coarse
 * transposed map); any pointer may be NULL. */
int ecm2_transfer_info(const ecm2_transfer *t, int *ne, int *order_lo, int *order_hi, int *ndofs_lo, int *ndofs_hi,
                       long *plan_bytes);
void ecm2_transfer_destroy(ecm2_transfer *t);
/* Multigrid(operators, smoothers, prolongations) (fem/multigrid.cpp:234-244) with the essential rows and columns of
 * the prolongations removed as GeometricMultigrid does (fem/multigrid.cpp:296-309): levels 0 (coarsest) ..
 * nlevels - 1; ops[k], smoothers[k] (built by the caller on ops[k] with ess[k]) and ess[k] (device int
 * [n_ess[k]], copied) per level, transfers[k] from level k to k + 1 (nlevels - 1 of them); pre and post smoothing
 * counts (the reference's defaults 1, 1).  V-cycle.  Sizes that do not chain or nlevels < 1: ECM2_ERR_ARG;
 * operators whose dots need communication, and a loopback group (ecm2_operator_from_par_group: its vectors are the
 * members' concatenated true vectors, not the L-vectors the transfers and essential lists number):
 * ECM2_ERR_UNSUPPORTED.  Every array holds nlevels entries (transfers: nlevels - 1); everything passed in must
 * outlive it. */
typedef struct ecm2_multigrid ecm2_multigrid;
int ecm2_multigrid_create(int nlevels, ecm2_operator *const *ops, ecm2_smoother *const *smoothers,
                          ecm2_transfer *const *transfers, const int *const *ess, const int *n_ess, int pre, int post,
                          ecm2_multigrid **out);
/* The coarsest level's solve: max_iter > 0: a constrained Jacobi-PCG from a zero guess with rel_tol and max_iter
 * (examples/ex26.cpp: sqrt(1e-4), 200); max_iter = 0: the level's smoother applied once (Multigrid's smoother at
 * level 0, fem/multigrid.cpp:179-186), the default. */
int ecm2_multigrid_set_coarse_pcg(ecm2_multigrid *mg, double rel_tol, int max_iter);
/* MultigridBase::Mult (fem/multigrid.cpp:106-145): y = one V-cycle (Cycle, SmoothingStep, :147-232) on x from a
 * zero guess; x, y distinct device vectors of the finest level's size, 16-byte aligned (ECM2_ERR_ARG otherwise).
 * Two calls are bitwise equal. */
int ecm2_multigrid_mult(ecm2_multigrid *mg, const double *x, double *y, void *stream);
void ecm2_multigrid_destroy(ecm2_multigrid *mg);
/* ecm2_operator_pcg_prec with prec = the cycle (CGSolver::Mult, solvers.cpp:869-1004; the finest level of A's
 * size, ECM2_ERR_ARG otherwise; A a loopback group: ECM2_ERR_UNSUPPORTED): the same stops, read-backs and results
 * as there. */
int ecm2_operator_pcg_mg(ecm2_operator *A, ecm2_multigrid *mg, const int *ess, int n_ess, const double *b, double *x,
                         double rel_tol, double abs_tol, int max_iter, int *iterations, double *final_norm,
                         void *stream);
/* ecm2_operator_pcg_mg with iterative_mode, as ecm2_operator_pcg_ex (CGSolver::Mult, solvers.cpp:875-884): the
 * outer CG starts from x; every cycle still starts from a zero guess (fem/multigrid.cpp:106-118).  0: that function. */
int ecm2_operator_pcg_mg_ex(ecm2_operator *A, ecm2_multigrid *mg, const int *ess, int n_ess, const double *b,
                            double *x, double rel_tol, double abs_tol, int max_iter, int *iterations,
                            double *final_norm, void *stream, int iterative_mode);
void ecm2_operator_destroy(ecm2_operator *op);

/* ------------------------------------------------------------------------ */
/* The device linear form: LinearForm + DomainLFIntegrator on the device path */
/* (LinearFormExtension::Assemble, fem/linearform_ext.cpp:20-68)              */
/* ------------------------------------------------------------------------ */
typedef struct ecm2_linear_form ecm2_linear_form;
/* Linear forms only: the RF Joule heat of a potential phi on the form's space,
 *   f = sigma0 (1 + slope (T - t_ref)) |grad phi|^2
 * (GradientGridFunctionCoefficient into InnerProductCoefficient, fem/coefficient.hpp:872, :1760;
 * JouleHeatingCoefficient::Eval, miniapps/electromagnetics/joule_solver.cpp:898): data = phi's device
 * L-vector, params[0..2] = (sigma0, slope, t_ref), data2 = T's device L-vector or NULL (sigma = sigma0).
 * A bilinear form refuses it (ECM2_ERR_ARG). */
#define ECM2_COEFF_JOULE 11
/* Host only: DomainLFIntegrator(Q, a = 2, b = 0) integrates with the rule of order a p + b = 2 p
 * (lininteg.hpp:116), i.e. p + 1 Gauss-Legendre points per direction (intrules.cpp:1181-1200). */
int ecm2_linear_form_default_q1d(int order);
/* LinearForm(fes) + LinearFormExtension (linearform.hpp, linearform_ext.cpp:18): gather_map as
 * ecm2_pa_form_create; q1d <= 0 selects the default above.  Kernels exist for order 1..4 with
 * q1d = order + 1 or order + 2 (DomainLFIntegrator's specialisations, lininteg_domain.cpp:104-115,
 * plus the forms' order 1, q1d 3 rule): anything else is ECM2_ERR_UNSUPPORTED. */
int ecm2_linear_form_create(int ne, int order, int ndofs, const int *gather_map, int q1d, ecm2_linear_form **out);
/* Geometry, as ecm2_pa_form_set_element_nodes / _set_jacobians (the last call wins; the Jacobians
 * must stay valid for as long as the form is assembled): GeometricFactors DETERMINANTS / JACOBIANS
 * (lininteg_domain.cpp:38-41) are evaluated in the kernel, never stored. */
int ecm2_linear_form_set_element_nodes(ecm2_linear_form *lf, const double *enodes /* host [ne][3][8] */);
int ecm2_linear_form_set_jacobians(ecm2_linear_form *lf, const double *J /* device, NQ x 3 x 3 x NE */);
/* Element attributes for marked integrators (Mesh::GetAttribute), host [ne]. */
int ecm2_linear_form_set_attributes(ecm2_linear_form *lf, const int *attr /* host [ne] */);
/* LinearForm::AddDomainIntegrator(new DomainLFIntegrator(Q)[, elem_marker]) (linearform.hpp).
 * coeff_kind: ECM2_COEFF_CONSTANT (data[0], host), _QUAD (device [ne][nq]), _GRIDFUNC (device
 * L-vector), _GRIDFUNC_AFFINE (device L-vector, params = scale, slope, t_ref) or _JOULE (above);
 * data2 is NULL except for _JOULE.  Vector and matrix kinds (and _GRIDFUNC_PERFUSION) are
 * ECM2_ERR_ARG.  marker: host [n_marker], 0 / 1 per attribute (an excluded element contributes
 * zeros, DLFEvalAssemble3D's markers[e] == 0), NULL: all elements.  Device pointers must stay valid
 * for as long as the form is assembled: every assemble re-reads them. */
int ecm2_linear_form_add_domain_integrator(ecm2_linear_form *lf, int coeff_kind, const double *data,
                                           const double *data2, const double *params, const int *marker,
                                           int n_marker);
/* LinearForm::Assemble -> LinearFormExtension::Assemble (linearform_ext.cpp:20-68): b = the sum of
 * the integrators in the order they were added (the first's R^T stores, the later ones add,
 * :64-67).  No atomics: two calls on the same inputs give bitwise equal vectors. */
int ecm2_linear_form_assemble(ecm2_linear_form *lf, double *b /* device [ndofs], overwritten */, void *stream);
/* LinearForm::AddBoundaryIntegrator(new BoundaryLFIntegrator(g)[, bdr_marker]): the boundary loop of
 * LinearFormExtension::Assemble (fem/linearform_ext.cpp:70-111: markers[e] = attr[e] > 0 &&
 * marker[attr[e] - 1], each integrator's face vectors transposed and added into b after the domain
 * integrators) and BoundaryLFIntegrator::AssembleDevice + BLFEvalAssemble3D
 * (fem/integ/lininteg_boundary.cpp:74-153, 214-228).  set_boundary: as ecm2_pa_form_set_boundary;
 * q1d <= 0 selects the integrator's default rule of order a p + b, a = b = 1 (lininteg.hpp:200):
 * (p + 1) / 2 + 1 points per direction; that, p + 1 and p + 2 are supported.  set_boundary_detj:
 * FaceGeometricFactors::detJ (mesh/mesh.cpp:15275-15334), device [nbe][q1d^2], read at every assemble.
 * coeff_kind: ECM2_COEFF_CONSTANT (data[0], host) or _QUAD (device [nbe][q1d^2], boundary element
 * order), anything else ECM2_ERR_ARG.  A form with boundary integrators only still overwrites b. */
int ecm2_linear_form_set_boundary(ecm2_linear_form *lf, int nbe, const int *bdr_map, const int *bdr_attr,
                                  const double *bdr_nodes, int q1d);
int ecm2_linear_form_set_boundary_detj(ecm2_linear_form *lf, const double *detj);
int ecm2_linear_form_add_boundary_integrator(ecm2_linear_form *lf, int coeff_kind, const double *data,
                                             const int *marker, int n_marker);
/* Introspection (any output may be NULL). */
int ecm2_linear_form_info(const ecm2_linear_form *lf, int *ne, int *ndofs, int *d1d, int *q1d, int *n_integrators);
/* ~LinearForm. */
void ecm2_linear_form_destroy(ecm2_linear_form *lf);

/* ------------------------------------------------------------------------ */
/* Cell death: the lesion state on the device                                 */
/* ------------------------------------------------------------------------ */
/* The last stage of an ablation simulation: which tissue died.  The model is the application's, not the
 * reference library's, so nothing here cites it; this comment is the model's statement.
 *
 * State.  Each dof holds three fractions N (native), U (unfolded, still reversible) and D (dead),
 * N + U + D = 1.
 * Rates.  k_i(T) = A_i exp(-dE_i / (R T_K)), i = 1..3, R = 8.31446261815324 J/(mol K), T_K = T + t_offset
 * (a field in degrees Celsius: t_offset = 273.15; a kelvin field: 0); A_i >= 0 [1/s] and dE_i >= 0 [J/mol] are
 * the caller's (A_i <= 1e150: the discriminant below squares the rates).
 * Kinetics.  N' = -k1 N + k2 U,  U' = k1 N - (k2 + k3) U,  D' = k3 U.
 *
 * ECM2_CELLDEATH_THREE_STATE: over a step of length dt with T frozen the update is the exact propagator of this
 * linear system -- not an ODE scheme: no stability limit, and a step of dt equals two steps of dt / 2.  The
 * eigenvalues are real and non-positive: with a, b, c = k1, k2, k3 and sigma = a + b + c the discriminant is
 * (2 delta)^2 = (a - c)^2 + b^2 + 2 b (a + c), lambda_- = -(sigma / 2 + delta), lambda_+ = a c / lambda_-.
 *   exp(M dt) = e^{lambda_- dt} I + g (M - lambda_- I),  g = e^{lambda_+ dt} (-expm1(-2 delta dt)) / (2 delta)
 * (no sinh: nothing overflows at 95 C and dt = 300 s); every quotient takes its limit where its denominator is
 * zero, so an entry whose rates are all zero (A_i = 0, or T_K so small that the exponentials underflow) is left
 * bitwise unchanged, and any single A_i = 0 works.  D is never recomputed as 1 - N - U: it advances by
 * dD = k3 int U dt >= 0 (through psi(l) = expm1(l dt) / l and G = (psi(lambda_+) - psi(lambda_-)) / (2 delta),
 * taken in the equal form (g - psi(lambda_-)) / lambda_+ wherever |lambda_+| >= 2 delta, so that nothing is divided
 * by a small 2 delta near a double eigenvalue), clamped at 0 from below, so D never decreases and N, U >= 0.  The
 * absolute error of every fraction is a few u (1 + dE / (R T_K)) per step; the relative error of a
 * small increment dD is not bounded.  rate * dt may overflow: everything then dies, nothing turns NaN.
 *
 * ECM2_CELLDEATH_ARRHENIUS: the classical one-integral damage, Omega += dt A_1 exp(-dE_1 / (R T_K)), stored in
 * U; D = 1 - exp(-Omega) (formed with expm1, never below the D passed in), N = 1 - D.  Only A_1, dE_1 are read.
 *
 * Temperature over the step.  The caller passes T0 and optionally T1, the field at the start and at the end of
 * the heat step, and nsub >= 1: substep m of length dt / nsub uses T0 + (m + 1/2) / nsub (T1 - T0); T1 == NULL
 * freezes T0 for every substep.  An entry whose T_K is non-finite or <= 0 at any substep is left unchanged and
 * counted. */
#define ECM2_CELLDEATH_THREE_STATE 0
#define ECM2_CELLDEATH_ARRHENIUS 1
typedef struct ecm2_celldeath ecm2_celldeath;
/* A state of n entries (one rank's dofs: the update is per dof, a distributed caller makes one per rank).
 * An unknown model, a negative or non-finite parameter, A_i > 1e150, a non-finite t_offset or n < 1:
 * ECM2_ERR_ARG, before a device is asked for; without a device: ECM2_ERR_HIP. */
int ecm2_celldeath_create(int model, const double params[6] /* A1, dE1, A2, dE2, A3, dE3 */, double t_offset, int n,
                          ecm2_celldeath **out);
/* One step: N, U, D (device [n]) in place from T0 and T1 (device [n]; T1 NULL: T0 frozen).  Checked before
 * anything is enqueued (ECM2_ERR_ARG): nsub < 1; a negative or non-finite dt; a vector that is not 16-byte
 * aligned (two entries per access, as ecm2_operator_bicgstab's x); T0 or T1 overlapping a state vector; state
 * vectors that overlap.  dt = 0 is the identity.  invalid (host, optional) receives the number of entries left
 * unchanged for their T_K; reading it back synchronises the stream, NULL does not (and is what a captured
 * stream needs).  No atomics: two steps on the same inputs are bitwise equal.  One handle serves one stream
 * at a time (it owns the partial sums' workspace). */
int ecm2_celldeath_step(ecm2_celldeath *h, const double *T0, const double *T1 /* NULL */, double dt, int nsub,
                        double *N, double *U, double *D, int *invalid /* NULL: not read back, no sync */,
                        void *stream);
/* out (host) = sum_i w_i D_i, sum_i w_i [D_i >= theta], sum_i w_i in one read of w and D (device [n], 16-byte
 * aligned).  With w the assembled linear form of the constant 1 (ecm2_linear_form_assemble) these are the dead
 * volume, the lesion volume and |Omega|.  Two-pass, a fixed summation order (bitwise reproducible);
 * synchronises the stream.  Across ranks the caller adds the ranks' sums (with w zeroed on dofs it does not own). */
int ecm2_celldeath_measure(ecm2_celldeath *h, const double *D, const double *w, double theta, double out[3],
                           void *stream);
/* Introspection (any output may be NULL). */
int ecm2_celldeath_info(const ecm2_celldeath *h, int *model, int *n, double params[6], double *t_offset);
void ecm2_celldeath_destroy(ecm2_celldeath *h);

/* ------------------------------------------------------------------------ */
/* Distributed form: ParBilinearForm / RAPOperator(P, A, P) over RCCL          */
/* ------------------------------------------------------------------------ */
typedef struct ecm2_partition ecm2_partition;

/* Mesh::CartesianPartitioning along z (mesh/mesh.cpp:8966) of a lexicographic Cartesian
 * mesh: elem_rank host [ne]. */
int ecm2_partition_slabs_z(const ecm2_mesh *m, int nranks, int *elem_rank);
/* Not a reference interface (the reference partitions with METIS or CartesianPartitioning):
 * equal runs of whole cell^3 element bricks of a Cartesian mesh in lexicographic brick order,
 * so that an owned-elements (ECM2_DECOMP_RAP) rank holds only whole bricks of the fused
 * kernels' blocks (balanced to one brick; measured against z-slabs in DESIGN.md §6).
 * elem_rank host [ne]. */
int ecm2_partition_bricks(const ecm2_mesh *m, int nranks, int cell, int *elem_rank);
/* Per-rank local space of a global H1 space and an element partition (ParMesh +
 * ParFiniteElementSpace, pmesh.hpp:33, pfespace.cpp:1389-1418): local L-vector
 * [owned | ghost], owner = lowest touching rank, local elements [interior | boundary],
 * neighbour exchange lists in the DeviceConformingProlongationOperator sense.  m (may be
 * NULL): when it is a Cartesian mesh the local element groups are put in brick order. */
int ecm2_partition_create(const ecm2_h1space *s, const ecm2_mesh *m, const int *elem_rank, int rank,
                          int nranks, ecm2_partition **out);
/* As ecm2_partition_create with a choice of decomposition: ECM2_DECOMP_RAP (the
 * reference's: local elements = owned elements, Mult = P, local PA, P^T) or
 * ECM2_DECOMP_OVERLAP (local elements = owned elements + every element touching an owned
 * dof, Mult = P, local PA; no P^T -- one exchange per Mult instead of two, the ghost
 * elements' outputs to non-owned dofs discarded; same operator). */
#define ECM2_DECOMP_RAP 0
#define ECM2_DECOMP_OVERLAP 1
int ecm2_partition_create_ex(const ecm2_h1space *s, const ecm2_mesh *m, const int *elem_rank, int rank,
                             int nranks, int decomposition, ecm2_partition **out);
/* Decomposition and the number of elements the rank owns (ne_local minus ghost elements). */
int ecm2_partition_decomposition(const ecm2_partition *p, int *decomposition, int *ne_owned);
int ecm2_partition_info(const ecm2_partition *p, int *ne_local, int *ne_interior, int *n_owned,
                        int *n_ghost, int *n_nbrs, int *n_send);
/* Any output may be NULL. elems [ne_local] (global ids, local order), local_to_global
 * [n_owned+n_ghost], gather_map [ne_local][nd] (local), nbrs [n_nbrs], send_off / recv_off
 * [n_nbrs+1], send_idx [n_send] (owned local indices). */
int ecm2_partition_get(const ecm2_partition *p, int *elems, int *local_to_global, int *gather_map,
                       int *nbrs, int *send_off, int *send_idx, int *recv_off);
/* The exchange schedule both transports consume (no reference counterpart; the reference's
 * per-neighbour MPI_Isend/Irecv of DeviceConformingProlongationOperator, pfespace.cpp:
 * 5394-5440 / 5496-5532, in one list): transpose = 0 for P (owners -> ghost copies), 1 for
 * P^T.  Rows of 5 ints (peer, send, buffer, offset, count), buffer 0 = the true vector x,
 * 1 = the packed send buffer [n_send], 2 = the ghost block of x [n_ghost], 3 = the ghost
 * block of y, 4 = the P^T receive buffer [n_send].  Two-call pattern: out may be NULL to
 * query *count.  Host only. */
int ecm2_partition_exchange_schedule(const ecm2_partition *p, int transpose, int *out, int *count);
/* ~ParFiniteElementSpace / ~ParMesh of the local view. */
void ecm2_partition_destroy(ecm2_partition *p);

/* ncclGetUniqueId (128 bytes) for ecm2_par_form_create; broadcast it to all ranks (the
 * reference's communicator is the ParMesh's MPI_Comm, pmesh.hpp:33). */
int ecm2_rccl_unique_id(unsigned char *id128);
/* Transport self-test (no reference counterpart): a one-rank communicator sends n doubles to
 * itself with grouped ncclSend/ncclRecv, directly (graph = 0) or captured in a HIP graph and
 * replayed (graph = 1, what ecm2_par_form_mult does); *max_err = max |received - sent|. */
int ecm2_rccl_p2p_selftest(int graph, int n, double *max_err);
/* ParBilinearForm(pfes) + SetAssemblyLevel(PARTIAL) (pbilinearform.hpp, bilinearform.cpp:
 * 109-136) on the rank's local space.  enodes_local: host [ne_local][3][8] in the
 * partition's local element order.
 * rccl_id: 128-byte id (one process per GPU, ncclCommInitRank) or NULL for a member of an
 * in-process loopback group (ecm2_par_group_mult). */
int ecm2_par_form_create(const ecm2_partition *p, const double *enodes_local, int q1d,
                         const unsigned char *rccl_id, ecm2_par_form **out);
/* As ecm2_pa_form_add_integrator, on local data: QUAD -> device [ne_local][nq] in local
 * element order; GRIDFUNC_AFFINE -> device local L-vector [n_owned + n_ghost]. */
int ecm2_par_form_add_integrator(ecm2_par_form *f, int integrator, int coeff_kind,
                                 const double *data, const double *params);
/* As ecm2_pa_form_add_integrator_marked / ecm2_pa_form_set_attributes on the local elements
 * (attributes host [ne_local], the partition's local element order). */
int ecm2_par_form_add_integrator_marked(ecm2_par_form *f, int integrator, int coeff_kind, const double *data,
                                        const double *params, const int *marker, int n_marker);
int ecm2_par_form_set_attributes(ecm2_par_form *f, const int *attr_local);
/* As ecm2_pa_form_set_kernel (fused kernels only). */
int ecm2_par_form_set_kernel(ecm2_par_form *f, int kernel);
/* Brick mode of the local form (see ecm2_pa_form_set_bricks). */
int ecm2_par_form_set_bricks(ecm2_par_form *f, int bz);
/* Schedule of the distributed Mult (no reference counterpart; the reference overlaps its
 * MPI exchange with nothing, pfespace.cpp:5394-5532): ECM2_SCHEDULE_SERIAL (default) = the P
 * exchange, ONE apply launch over every local element, the shared-dof sums, all on the
 * caller's stream; ECM2_SCHEDULE_OVERLAP = interior elements on the caller's stream beside the
 * exchange + boundary elements on a high-priority comm stream.  graph: 1 = replay one captured
 * HIP graph per (x, y), 0 = direct launches, -1 = the schedule's default (serial: direct,
 * overlap: graph).  Before Assemble. */
#define ECM2_SCHEDULE_SERIAL 0
#define ECM2_SCHEDULE_OVERLAP 1
int ecm2_par_form_set_schedule(ecm2_par_form *f, int schedule, int graph);
/* Scatter mode of the local form (ECM2_SCATTER_*; see ecm2_pa_form_set_scatter). */
int ecm2_par_form_set_scatter(ecm2_par_form *f, int mode);
/* Geometry compression of the local form (see ecm2_pa_form_set_geometry_compression). */
int ecm2_par_form_set_geometry_compression(ecm2_par_form *f, int on);
/* ParBilinearForm::Assemble -> local PABilinearFormExtension::Assemble
 * (pbilinearform.cpp:475-511, bilinearform_ext.cpp:332-368). */
int ecm2_par_form_assemble(ecm2_par_form *f, void *stream);
/* RAPOperator::Mult (operator.hpp:977): y_true = P^T A P x_true; x_true, y_true device
 * [n_owned].  Grouped ncclSend/ncclRecv, then the local PA apply and the shared-dof sums on
 * `stream` (ECM2_SCHEDULE_SERIAL, the default); see ecm2_par_form_set_schedule. */
int ecm2_par_form_mult(ecm2_par_form *f, const double *x_true, double *y_true, void *stream);
/* RAPOperator::MultTranspose (operator.hpp:979): P^T A^T P = P^T A P (A symmetric). */
int ecm2_par_form_mult_transpose(ecm2_par_form *f, const double *x_true, double *y_true, void *stream);
/* ecm2_pa_form_addressing_info for the rank's local form (its interior blocks can be
 * lattice-addressed, those touching ghost dofs are not). */
int ecm2_par_form_addressing_info(const ecm2_par_form *f, int *lattice, int *n_units, long *n_runs);
/* All subdomains of one partition in this process on one GPU (exchange by device copies that
 * follow the members' exchange schedules). */
int ecm2_par_group_mult(ecm2_par_form *const *forms, int n, const double *const *x_true,
                        double *const *y_true, void *stream);
/* Transport test (no reference counterpart): ecm2_par_group_mult with every exchange row
 * issued through RCCL -- a one-rank communicator (created on the first call, which must not be
 * inside a stream capture) ncclSend's each peer's send row to itself and ncclRecv's it into
 * the matching receive row, grouped, on `stream` (capturable).  Exercises the row buffers,
 * offsets and counts of ecm2_par_form_mult's grouped exchange on one GPU.  Serial schedule. */
int ecm2_par_group_mult_rccl(ecm2_par_form *const *forms, int n, const double *const *x_true,
                             double *const *y_true, void *stream);
/* One member's rows of the loopback group's operator (measurement of a rank's Mult on its own
 * GPU; no reference counterpart): y_true[member] = (A x)[member's true dofs], running exactly
 * the stages one RCCL rank runs (interior elements on `stream`, the P exchange -- here device
 * copies from the peers' x -- and the boundary elements on the member's comm stream, then the
 * shared-dof sums); the other members' y are not written.  Packed sends (non-slab partitions)
 * and, with RAP (serial schedule), the P^T receive copy the peers' buffers as their last
 * ecm2_par_group_mult left them (run one group Mult on the same x first).
 * ECM2_ERR_UNSUPPORTED otherwise (RAP with the overlapped schedule). */
int ecm2_par_group_mult_member(ecm2_par_form *const *forms, int n, int member, const double *const *x_true,
                               double *const *y_true, void *stream);
/* ParBilinearForm::AssembleDiagonal on the true dofs (local PA diagonal + P^T). */
int ecm2_par_form_assemble_diagonal(ecm2_par_form *f, double *d_true, void *stream);
int ecm2_par_group_diagonal(ecm2_par_form *const *forms, int n, double *const *d_true, void *stream);
/* Measurement and introspection (no reference counterpart): HIP-event timing of the local
 * apply kernels, SURVEY §8(d) bytes of the local form, true size and resolved kernel. */
int ecm2_par_form_timing(ecm2_par_form *f, int enable);
int ecm2_par_form_timing_get(ecm2_par_form *f, double *total_ms, long *launches);
int ecm2_par_form_algorithmic_bytes(const ecm2_par_form *f, double *bytes);
int ecm2_par_form_qdata_bytes(const ecm2_par_form *f, double *bytes);
/* Whether the local form's last Assemble took the coefficient snapshot
 * (ecm2_pa_form_coefficient_snapshot). */
int ecm2_par_form_coefficient_snapshot(const ecm2_par_form *f, int *on);
/* Quadrature-data layout of the local form (ECM2_QLAYOUT_*), after assemble. */
int ecm2_par_form_layout(const ecm2_par_form *f, int *layout);
int ecm2_par_form_info(const ecm2_par_form *f, int *n_true, int *kernel);
/* ~ParBilinearForm. */
void ecm2_par_form_destroy(ecm2_par_form *f);

#ifdef __cplusplus
}
#endif
#endif /* ECM2_PA_H */
