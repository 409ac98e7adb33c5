! Driver of tools/make_golden_propags1.py: calls the reference's PROPCONNECT with IPROPAGS = 1, then PROPDOT (with GRADI) and PROPAGS1 on the cases of a
! stream file, and writes the tables and what the routines return.  It is built by oracle/ref_build.py::build_driver: the routines and the modules they use
! are the reference's own files, compiled unmodified in both precisions, behind the stand-ins of oracle/ref_stubs.F90; the driver holds no module of its own.
! The program fills the module variables the routines read (the USE lines of propags1.F90:88-105, propconnect.F90:34-44, propdot.F90:67-73 and
! gradi.F90:65-70): YOWMAP (IPER = 1, NGX, NGY, NLONRGG, ZDELLO, XDELLA, BLK2GLO), YOWSHAL (LLOCEANMASK from the sea points), YOWSPEC (the identity
! IJ2NEWIJ; NEWIJ2IJ is the identity too).
! Statements of MPL-bound routines the driver restates, single task, around the call of PROPCONNECT:
!   mpdecomp.F90 step 5 (:1264-1300)  PROPCONNECT's 0 ("a land point is neighbour") becomes the land index NSUP + 1 in KLAT, KLON, KRLAT, KRLON
!   mpdecomp.F90:1192-1254            CDR, SDR (NINF:NSUP+1, NANG; the land row 0) and PRQRT, the branch of one task (NPR = 1)
! It also writes SQRT2 = 2.0_JWRB*SIN(0.25_JWRB*PI) of propags1.F90:570 as the compiler evaluates it.
! PROPAGS1 and PROPDOT then run with the KLAT, KLON and WLAT of the input file (those of the propags_* fixtures: the tool requires PROPCONNECT's KLAT and
! KLON to equal them; its WLAT, formed from the rounded increments of the file, is recorded and not used) and with PROPCONNECT's rotated tables.
! The one routine the driver supplies in place of the reference's is the external CHECKCFL below, as tools/propags_driver.F90 does: it records its eleven
! arguments per (K, M = 1) instead of aborting.  build_driver cuts checkcfl.intfb.h from it.
! Input  (stream, little endian): N, NANG, NFRE_RED, NGY (int32); FR(NFRE_RED), SINTH(NANG), COSTH(NANG), then DELTH, R, ZPI, PI (real64); NLONRGG(NGY), IXLG(N),
!        KXLT(N), KLON(N,2), KLAT(N,2,2) (int32, 1-based, the land row is N+1); XDELLA, DELPHI (real64); ZDELLO(NGY), DELLAM(NGY), SINPH(NGY), COSPH(NGY), WLAT(N,2);
!        then cases, each led by an int32 1 (0 ends the file):
!          ICASE, IRGG, IREFRA, IDELPRO, LOBS (int32); DELLAM1, COSPHM1, DEPTH, U, V (N+1 each); CGROUP, OMOSNH2KD, WAVNUM (N+1,NFRE_RED each); with LOBS /= 0
!          OBSLAT, OBSLON, OBSRLAT, OBSRLON (N,NFRE_RED,2 each); F1(N+1,NANG,NFRE_RED)
!        Every real is representable in the working precision.
! Output (stream, real64: the working-precision results, widened): KLAT(N,2,2), KLON(N,2), KRLAT(N,2,2), KRLON(N,2,2), WLAT(N,2), WRLAT(N,2), WRLON(N,2) of
!        PROPCONNECT after step 5; CDR(N+1,NANG), SDR(N+1,NANG), PRQRT(N), SQRT2; per case F3(N,NANG,NFRE_RED), CFL(N,NANG,11), the number of CHECKCFL calls.
PROGRAM PROPAGS1_DRIVER
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  USE YOWCURR, ONLY : LLCHKCFL
  USE YOWFRED, ONLY : FR, DELTH, COSTH, SINTH
  USE YOWGRID, ONLY : DELPHI, DELLAM, SINPH, COSPH, CDR, SDR, PRQRT
  USE YOWMAP, ONLY : BLK2GLO, IPER, IRGG, XDELLA, ZDELLO, NLONRGG, NGX, NGY, NIBLO
  USE YOWPARAM, ONLY : NANG, NFRE, NFRE_RED
  USE YOWPCONS, ONLY : PI, ZPI, R
  USE YOWREFD, ONLY : THDD, THDC, SDOT
  USE YOWSHAL, ONLY : LLOCEANMASK
  USE YOWSPEC, ONLY : IJ2NEWIJ
  USE YOWSTAT, ONLY : IDELPRO, ICASE, IREFRA, IPROPAGS
  USE YOWUBUF, ONLY : KLAT, KLON, KRLAT, KRLON, WLAT, WRLAT, WRLON, OBSLAT, OBSLON, OBSRLAT, OBSRLON
  IMPLICIT NONE
#include "propconnect.intfb.h"
#include "propdot.intfb.h"
#include "propags1.intfb.h"
  INTEGER, PARAMETER :: R8 = SELECTED_REAL_KIND(13, 300)
  INTEGER, PARAMETER :: MAXP = 256, MAXK = 64
  REAL(KIND=R8) :: CFLREC(MAXP, MAXK, 11)
  INTEGER :: NCALL
  COMMON /PGREC/ CFLREC, NCALL
  INTEGER(KIND=JWIM) :: N, OP, LOBS, IJ, K, JH, NLAND
  INTEGER(KIND=JWIM), ALLOCATABLE, TARGET :: KXLT(:), IXLG(:)
  INTEGER(KIND=JWIM), ALLOCATABLE :: NEWIJ2IJ(:), KLON_IN(:,:), KLAT_IN(:,:,:)
  REAL(KIND=R8) :: S(4), D8(2)
  REAL(KIND=R8), ALLOCATABLE :: A8(:), G8(:), W8(:,:), P8(:,:), E8(:,:,:), O8(:,:,:,:), F8(:,:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: F1(:,:,:), F3(:,:,:), P(:,:), E(:,:,:)
  REAL(KIND=JWRB) :: SQRT2O2, SQRT2, A, B, THETAMAX, SINTHMAX, DELTA
  CHARACTER(LEN=512) :: FIN, FOUT

  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  OPEN(11, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(12, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  READ(11) N, NANG, NFRE_RED, NGY
  IF (N > MAXP .OR. NANG > MAXK) ERROR STOP 'SIZE'
  NFRE = NFRE_RED
  NIBLO = N
  NLAND = N + 1
  ALLOCATE(FR(NFRE_RED), SINTH(NANG), COSTH(NANG), A8(NFRE_RED))
  READ(11) A8
  FR = REAL(A8, JWRB)
  DEALLOCATE(A8)
  ALLOCATE(A8(NANG))
  READ(11) A8
  SINTH = REAL(A8, JWRB)
  READ(11) A8
  COSTH = REAL(A8, JWRB)
  READ(11) S
  DELTH = REAL(S(1), JWRB)
  R = REAL(S(2), JWRB)
  ZPI = REAL(S(3), JWRB)
  PI = REAL(S(4), JWRB)
  ALLOCATE(NLONRGG(NGY), IXLG(N), KXLT(N), KLON_IN(N,2), KLAT_IN(N,2,2))
  READ(11) NLONRGG, IXLG, KXLT, KLON_IN, KLAT_IN
  ALLOCATE(KLON(N,2), KLAT(N,2,2), KRLAT(N,2,2), KRLON(N,2,2), WLAT(N,2), WRLAT(N,2), WRLON(N,2))
  ALLOCATE(OBSLAT(N,NFRE_RED,2), OBSLON(N,NFRE_RED,2), OBSRLAT(N,NFRE_RED,2), OBSRLON(N,NFRE_RED,2))
  BLK2GLO%KXLT => KXLT
  BLK2GLO%IXLG => IXLG
  READ(11) D8
  XDELLA = REAL(D8(1), JWRB)
  DELPHI = REAL(D8(2), JWRB)
  ALLOCATE(ZDELLO(NGY), DELLAM(NGY), SINPH(NGY), COSPH(NGY), G8(NGY), W8(N,2))
  READ(11) G8
  ZDELLO = REAL(G8, JWRB)
  READ(11) G8
  DELLAM = REAL(G8, JWRB)
  READ(11) G8
  SINPH = REAL(G8, JWRB)
  READ(11) G8
  COSPH = REAL(G8, JWRB)
  READ(11) W8

  ! ---- the tables: PROPCONNECT as mpdecomp.F90 calls it, on one task
  NGX = MAXVAL(NLONRGG)
  IPER = 1
  IRGG = 1
  IPROPAGS = 1
  ALLOCATE(LLOCEANMASK(NGX,NGY), IJ2NEWIJ(0:N+1), NEWIJ2IJ(N))
  LLOCEANMASK = .FALSE.
  DO IJ = 1, N
    LLOCEANMASK(IXLG(IJ), KXLT(IJ)) = .TRUE.
    NEWIJ2IJ(IJ) = IJ
  ENDDO
  DO IJ = 0, N + 1
    IJ2NEWIJ(IJ) = IJ
  ENDDO
  CALL PROPCONNECT(1_JWIM, N, NEWIJ2IJ)
  ! mpdecomp.F90 step 5
  WHERE (KLAT == 0) KLAT = NLAND
  WHERE (KLON == 0) KLON = NLAND
  WHERE (KRLAT == 0) KRLAT = NLAND
  WHERE (KRLON == 0) KRLON = NLAND
  ! mpdecomp.F90:1192-1254, NPR = 1
  ALLOCATE(CDR(1:N+1,NANG), SDR(1:N+1,NANG), PRQRT(1:N))
  SQRT2O2=SIN(0.25_JWRB*PI)
  DO K=1,NANG
    CDR(NLAND,K) = 0.0_JWRB
    SDR(NLAND,K) = 0.0_JWRB
  ENDDO
  DO IJ=1,N
    JH = BLK2GLO%KXLT(IJ)
    DO K=1,NANG
      A=SQRT2O2*COSTH(K)*COSPH(JH)
      B=SQRT2O2*SINTH(K)
      CDR(IJ,K)=A-B
      SDR(IJ,K)=A+B
    ENDDO
  ENDDO
  IF (IRGG == 1) THEN
    DO IJ=1,N
      JH = BLK2GLO%KXLT(IJ)
      THETAMAX=ATAN2(1.0_JWRB,COSPH(JH))
      SINTHMAX=SIN(THETAMAX)
      DELTA=COSPH(JH)/(SINTHMAX*(1.0_JWRB+COSPH(JH)**2))
      PRQRT(IJ)=MIN(0.5_JWRB,DELTA)
    ENDDO
  ELSE
    DO IJ=1,N
      PRQRT(IJ)=0.5_JWRB
    ENDDO
  ENDIF
  SQRT2=2.0_JWRB*SIN(0.25_JWRB*PI)
  WRITE(12) REAL(KLAT, R8), REAL(KLON, R8), REAL(KRLAT, R8), REAL(KRLON, R8), REAL(WLAT, R8), REAL(WRLAT, R8), REAL(WRLON, R8)
  WRITE(12) REAL(CDR, R8), REAL(SDR, R8), REAL(PRQRT, R8), REAL(SQRT2, R8)
  ! the tables of the input file from here on
  KLAT = KLAT_IN
  KLON = KLON_IN
  WLAT = REAL(W8, JWRB)

  ALLOCATE(P8(N+1,5), P(N+1,5), E8(N+1,NFRE_RED,3), E(N+1,NFRE_RED,3), O8(N,NFRE_RED,2,4))
  ALLOCATE(F8(N+1,NANG,NFRE_RED), F1(N+1,NANG,NFRE_RED), F3(N+1,NANG,NFRE_RED))
  ALLOCATE(THDD(N,NANG), THDC(N,NANG), SDOT(N,NANG,NFRE_RED))
  LLCHKCFL = .TRUE.
  DO
    READ(11) OP
    IF (OP == 0) EXIT
    READ(11) ICASE, IRGG, IREFRA, IDELPRO, LOBS
    READ(11) P8, E8
    P = REAL(P8, JWRB)
    E = REAL(E8, JWRB)
    OBSLAT = 1.0_JWRB
    OBSLON = 1.0_JWRB
    OBSRLAT = 1.0_JWRB
    OBSRLON = 1.0_JWRB
    IF (LOBS /= 0) THEN
      READ(11) O8
      OBSLAT = REAL(O8(:,:,:,1), JWRB)
      OBSLON = REAL(O8(:,:,:,2), JWRB)
      OBSRLAT = REAL(O8(:,:,:,3), JWRB)
      OBSRLON = REAL(O8(:,:,:,4), JWRB)
    ENDIF
    READ(11) F8
    F1 = REAL(F8, JWRB)
    F3 = 0.0_JWRB
    THDD = 0.0_JWRB
    THDC = 0.0_JWRB
    SDOT = 0.0_JWRB
    CFLREC = 0.0_R8
    NCALL = 0
    ! propag_wam.F90:296-322: the dot terms with refraction, then the scheme
    IF (IREFRA /= 0) THEN
      CALL PROPDOT(1_JWIM, N, 1_JWIM, N, BLK2GLO, E(:,:,3), E(:,:,1), E(:,:,2), P(:,2), P(:,3), P(:,4), P(:,5), THDC, THDD, SDOT)
    ENDIF
    CALL PROPAGS1(F1, F3, 1_JWIM, N, 1_JWIM, N, BLK2GLO, P(:,3), E(:,:,1), E(:,:,2), P(:,1), P(:,2), P(:,4), P(:,5), .TRUE.)
    WRITE(12) REAL(F3(1:N,:,:), R8), CFLREC(1:N,1:NANG,:), REAL(NCALL, R8)
  ENDDO
  CLOSE(11)
  CLOSE(12)
END PROGRAM PROPAGS1_DRIVER

SUBROUTINE CHECKCFL (KIJS, KIJL, DEPTH, DTC, CFLEA, CFLWE, CFLNO, CFLSO, CFLNO2, CFLSO2, CFLTP, CFLTM, CFLOP, CFLOM)
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  IMPLICIT NONE
  INTEGER(KIND=JWIM), INTENT(IN) :: KIJS, KIJL
  REAL(KIND=JWRB), DIMENSION(KIJS:KIJL), INTENT(IN) :: DEPTH
  REAL(KIND=JWRB), DIMENSION(KIJS:KIJL), INTENT(IN) :: DTC
  REAL(KIND=JWRB), DIMENSION(KIJS:KIJL), INTENT(IN) :: CFLEA, CFLWE, CFLNO, CFLSO, CFLNO2
  REAL(KIND=JWRB), DIMENSION(KIJS:KIJL), INTENT(IN) :: CFLSO2, CFLTP, CFLTM, CFLOP, CFLOM
  INTEGER, PARAMETER :: R8 = SELECTED_REAL_KIND(13, 300)
  INTEGER, PARAMETER :: MAXP = 256, MAXK = 64
  REAL(KIND=R8) :: CFLREC(MAXP, MAXK, 11)
  INTEGER :: NCALL
  COMMON /PGREC/ CFLREC, NCALL
  INTEGER(KIND=JWIM) :: IJ, K
  NCALL = NCALL + 1
  K = NCALL
  IF (K > MAXK) ERROR STOP 'CHECKCFL CALLS'
  DO IJ = KIJS, KIJL
    CFLREC(IJ,K,1) = REAL(DTC(IJ), R8)
    CFLREC(IJ,K,2) = REAL(CFLEA(IJ), R8)
    CFLREC(IJ,K,3) = REAL(CFLWE(IJ), R8)
    CFLREC(IJ,K,4) = REAL(CFLNO(IJ), R8)
    CFLREC(IJ,K,5) = REAL(CFLSO(IJ), R8)
    CFLREC(IJ,K,6) = REAL(CFLNO2(IJ), R8)
    CFLREC(IJ,K,7) = REAL(CFLSO2(IJ), R8)
    CFLREC(IJ,K,8) = REAL(CFLTP(IJ), R8)
    CFLREC(IJ,K,9) = REAL(CFLTM(IJ), R8)
    CFLREC(IJ,K,10) = REAL(CFLOP(IJ), R8)
    CFLREC(IJ,K,11) = REAL(CFLOM(IJ), R8)
  ENDDO
END SUBROUTINE CHECKCFL
